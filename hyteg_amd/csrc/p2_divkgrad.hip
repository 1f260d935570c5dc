// C-ABI entry points of the variable-coefficient P2 diffusion operator -div( k grad u ) with a P2 coefficient on one macro-cell:
// the seam of the generated operatorgeneration::P2ElementwiseDivKGrad (apply / computeInverseDiagonalOperatorValues of module
// hyteg_operators; in-tree use: tests/hyteg/convergence/ElementwiseDivKGradCGConvergenceTest.cpp:192-221).  Kernels and the
// arithmetic: kernels_p2_divkgrad.hpp.
#include <atomic>
#include <cmath>

#include "element_matrices.hpp"
#include "kernels_p2_divkgrad.hpp"

namespace {

// first level whose inner DoFs are computed by the inner form (compile-time micro-cell lists); below, and for the boundary DoFs of
// every level, the gather form.  Measured per level in one run (tools/bench_kernels.py --only p2-divkgrad): the inner
// form is a long dependent chain per thread and loses to the eight-lane gather form at levels 4 and 5 (45 against 18 us, 48 against
// 26 us); it wins from level 6 (71 against 80 us, 310 against 412 us at level 7), beyond the spread of five repeats.
constexpr int       kInnerMinLevelDefault = 6;
std::atomic< int >& inner_min_level()
{
   static std::atomic< int > v( env_int( "HYTEG_HIP_P2_DIVKGRAD_INNER_MIN_LEVEL", kInnerMinLevelDefault ) );
   return v;
}

int validate( const char* who, const double* dstV, const double* dstE, const double* srcV, const double* srcE, const double* kV, const double* kE, int level,
              const double* geometry, int update )
{
   const std::string w( who );
   HH_REQUIRE( dstV && dstE && srcV && srcE && kV && kE && geometry, w + ": null pointer" );
   HH_REQUIRE( level >= 0 && level <= kP2DivKGradMaxLevel, w + ": level out of range [0,8]" );
   for ( const double* d : { dstV, dstE } )
      HH_REQUIRE( d != srcV && d != srcE && d != kV && d != kE, w + ": a written array must not alias src or k" );
   HH_REQUIRE( update == HYTEG_HIP_REPLACE || update == HYTEG_HIP_ADD, w + ": bad update type" );
   return HYTEG_HIP_OK;
}

DkArgs make_args( double* dstV, double* dstE, const double* srcV, const double* srcE, const double* kV, const double* kE, int level, const double* geometry,
                  double alpha, int update, unsigned mask, unsigned kinds )
{
   DkArgs A{};
   A.dstV = dstV, A.dstE = dstE, A.srcV = srcV, A.srcE = srcE, A.kV = kV, A.kE = kE, A.alpha = alpha;
   A.N = ( 1 << level ) + 1, A.update = update, A.diag = 0, A.mask = mask, A.kinds = kinds;
   for ( int t = 0; t < 6; ++t )
      for ( int p = 0; p < 10; ++p )
         A.W.g[t][p] = geometry[10 * t + p];
   return A;
}

// the gather form on the DoFs of A.mask: all entries of the kinds' arrays if an inner DoF is asked for, else the boundary walk.  Eight
// lanes per DoF where the launch is latency-bound (the boundary walk, and all DoFs up to level 5); one lane per DoF above, where
// repeating the index decode eight times costs more than the round trips (tools/bench_kernels.py --only p2-divkgrad)
constexpr int kGatherLanes = 8, kGatherLanesMaxLevel = 5;
int launch_gather( const DkArgs& A, int level, hipStream_t s )
{
   DkGatherArgs G;
   G.A = A, G.T = tables();
   if ( A.mask & HYTEG_HIP_MASK_INNER )
   {
      const unsigned dofs = tet32( (unsigned) A.N );
      if ( level <= kGatherLanesMaxLevel )
         hipLaunchKernelGGL( ( p2_divkgrad_gather_kernel< true, kGatherLanes > ), dim3( ( dofs * kGatherLanes + kThreads - 1 ) / kThreads, 8 ),
                             dim3( kThreads ), 0, s, G );
      else
         hipLaunchKernelGGL( ( p2_divkgrad_gather_kernel< true, 1 > ), dim3( ( dofs + kThreads - 1 ) / kThreads, 8 ), dim3( kThreads ), 0, s, G );
   }
   else
   {
      const unsigned dofs = (unsigned) ( 4 * tri( A.N ) );
      hipLaunchKernelGGL( ( p2_divkgrad_gather_kernel< false, kGatherLanes > ), dim3( ( dofs * kGatherLanes + kThreads - 1 ) / kThreads, 8 ),
                          dim3( kThreads ), 0, s, G );
   }
   HH_CHECK_HIP( hipGetLastError() );
   return HYTEG_HIP_OK;
}

} // namespace

extern "C" {

HYTEG_HIP_API int hyteg_hip_p2_elementwise_divkgrad_geometry( const double* macro_vertex_coords, int level, double* geometry )
{
   const char* who = "p2_elementwise_divkgrad_geometry";
   HH_REQUIRE( macro_vertex_coords && geometry, std::string( who ) + ": null pointer" );
   HH_REQUIRE( level >= 0 && level <= kP2DivKGradMaxLevel, std::string( who ) + ": level out of range [0,8]" );
   double cc[4][3];
   for ( int v = 0; v < 4; ++v )
      for ( int r = 0; r < 3; ++r )
         cc[v][r] = macro_vertex_coords[3 * v + r];
   for ( int t = 0; t < 6; ++t )
   {
      double       c[4][3], g[4][3];
      elmat::micro_cell_coords( cc, int64_t( 1 ) << level, t, c );
      const double V = elmat::gradients( c, g );
      HH_REQUIRE( V > 0.0 && std::isfinite( V ), std::string( who ) + ": degenerate macro-cell" );
      for ( int a = 0; a < 4; ++a )
         for ( int b = a; b < 4; ++b )
            geometry[10 * t + kDkPair[a][b]] = V * ( g[a][0] * g[b][0] + g[a][1] * g[b][1] + g[a][2] * g[b][2] ) / 840.0;
   }
   return HYTEG_HIP_OK;
}

HYTEG_HIP_API int hyteg_hip_p2_elementwise_divkgrad_apply_cell_kinds( double*            dst_vertex,
                                                                      double*            dst_edge,
                                                                      const double*      src_vertex,
                                                                      const double*      src_edge,
                                                                      const double*      k_vertex,
                                                                      const double*      k_edge,
                                                                      int                level,
                                                                      const double*      geometry,
                                                                      double             alpha,
                                                                      int                update,
                                                                      unsigned           mask,
                                                                      unsigned           kind_mask,
                                                                      hyteg_hip_stream_t stream )
{
   const int rc = validate( "p2_elementwise_divkgrad_apply_cell", dst_vertex, dst_edge, src_vertex, src_edge, k_vertex, k_edge, level, geometry, update );
   if ( rc != HYTEG_HIP_OK )
      return rc;
   mask &= HYTEG_HIP_MASK_ALL;
   kind_mask &= 0xFFu;
   if ( mask == 0 || kind_mask == 0 )
      return HYTEG_HIP_OK;
   DkArgs     A     = make_args( dst_vertex, dst_edge, src_vertex, src_edge, k_vertex, k_edge, level, geometry, alpha, update, mask, kind_mask );
   const bool inner = ( mask & HYTEG_HIP_MASK_INNER ) && level >= 2 && level >= inner_min_level().load( std::memory_order_relaxed );
   if ( !inner )
      return launch_gather( A, level, as_stream( stream ) );
   if ( mask & HYTEG_HIP_MASK_SHELL )
   {
      DkArgs B = A;
      B.mask   = mask & HYTEG_HIP_MASK_SHELL;
      const int rs = launch_gather( B, level, as_stream( stream ) );
      if ( rs != HYTEG_HIP_OK )
         return rs;
   }
   const unsigned nb = ( tet32( (unsigned) A.N ) + kThreads - 1 ) / kThreads;
   if ( kind_mask & 1u )
      hipLaunchKernelGGL( p2_divkgrad_inner_vertex_kernel, dim3( nb ), dim3( kThreads ), 0, as_stream( stream ), A );
   if ( kind_mask & 0xFEu )
      hipLaunchKernelGGL( p2_divkgrad_inner_edge_kernel, dim3( nb, 7 ), dim3( kThreads ), 0, as_stream( stream ), A );
   HH_CHECK_HIP( hipGetLastError() );
   return HYTEG_HIP_OK;
}

HYTEG_HIP_API int hyteg_hip_p2_elementwise_divkgrad_apply_cell_gather( double*            dst_vertex,
                                                                       double*            dst_edge,
                                                                       const double*      src_vertex,
                                                                       const double*      src_edge,
                                                                       const double*      k_vertex,
                                                                       const double*      k_edge,
                                                                       int                level,
                                                                       const double*      geometry,
                                                                       double             alpha,
                                                                       int                update,
                                                                       unsigned           mask,
                                                                       unsigned           kind_mask,
                                                                       hyteg_hip_stream_t stream )
{
   const int rc = validate( "p2_elementwise_divkgrad_apply_cell_gather", dst_vertex, dst_edge, src_vertex, src_edge, k_vertex, k_edge, level, geometry, update );
   if ( rc != HYTEG_HIP_OK )
      return rc;
   mask &= HYTEG_HIP_MASK_ALL;
   kind_mask &= 0xFFu;
   if ( mask == 0 || kind_mask == 0 )
      return HYTEG_HIP_OK;
   return launch_gather( make_args( dst_vertex, dst_edge, src_vertex, src_edge, k_vertex, k_edge, level, geometry, alpha, update, mask, kind_mask ),
                         level, as_stream( stream ) );
}

HYTEG_HIP_API int hyteg_hip_p2_elementwise_divkgrad_diagonal_cell( double*            diag_vertex,
                                                                   double*            diag_edge,
                                                                   const double*      k_vertex,
                                                                   const double*      k_edge,
                                                                   int                level,
                                                                   const double*      geometry,
                                                                   hyteg_hip_stream_t stream )
{
   const int rc = validate( "p2_elementwise_divkgrad_diagonal_cell", diag_vertex, diag_edge, k_vertex, k_edge, k_vertex, k_edge, level, geometry,
                            HYTEG_HIP_REPLACE );
   if ( rc != HYTEG_HIP_OK )
      return rc;
   DkArgs A = make_args( diag_vertex, diag_edge, k_vertex, k_edge, k_vertex, k_edge, level, geometry, 1.0, HYTEG_HIP_REPLACE, HYTEG_HIP_MASK_ALL, 0xFFu );
   A.diag   = 1;
   return launch_gather( A, level, as_stream( stream ) );
}

HYTEG_HIP_API int hyteg_hip_p2_elementwise_divkgrad_set_inner_min_level( int level )
{
   const int before = inner_min_level().load();
   inner_min_level().store( level < 2 ? 2 : level );
   return before;
}

HYTEG_HIP_API int hyteg_hip_p2_elementwise_divkgrad_max_level( void ) { return kP2DivKGradMaxLevel; }
}
