// C-ABI entry points of the variable-viscosity P2 epsilon operator -div( 2 mu eps( u ) ) with a P2 viscosity on one macro-cell: the
// seam of operatorgeneration::P2ViscousBlockEpsilonOperator (apply / computeInverseDiagonalOperatorValues; the velocity block of
// operatorgeneration::P2P1StokesEpsilonOperator, whose mu = 1 case is the P2 half of
// tests/hyteg/convergence/ElementwiseEpsilonMinResConvergenceTest.cpp:156-163, 366-412).  Kernels and the arithmetic:
// kernels_p2_epsilon.hpp.
#include <atomic>
#include <cmath>

#include "element_matrices.hpp"
#include "kernels_p2_epsilon.hpp"

namespace {

// first level whose inner DoFs are computed by the inner form (compile-time micro-cell lists); below, and for the boundary DoFs of
// every level, the gather form.  Measured per level in one run (tools/bench_kernels.py --only p2-epsilon): the inner
// form is a long dependent chain per thread and loses to the gather form at levels 4 to 6 (73 against 21 us, 78 against 43 us,
// 139 against 117 us); it wins at level 7 (754 against 832 us), beyond the spread of five repeats.
constexpr int       kInnerMinLevelDefault = 7;
std::atomic< int >& inner_min_level()
{
   static std::atomic< int > v( env_int( "HYTEG_HIP_P2_EPSILON_INNER_MIN_LEVEL", kInnerMinLevelDefault ) );
   return v;
}

int validate( const char* who, double* const* dstV, double* const* dstE, const double* const* srcV, const double* const* srcE, const double* muV,
              const double* muE, int level, const double* geometry, int update )
{
   const std::string w( who );
   HH_REQUIRE( dstV && dstE && srcV && srcE && muV && muE && geometry, w + ": null pointer" );
   for ( int k = 0; k < 3; ++k )
      HH_REQUIRE( dstV[k] && dstE[k] && srcV[k] && srcE[k], w + ": null pointer" );
   HH_REQUIRE( level >= 0 && level <= kP2EpsilonMaxLevel, w + ": level out of range [0,8]" );
   const double* written[6] = { dstV[0], dstV[1], dstV[2], dstE[0], dstE[1], dstE[2] };
   for ( int a = 0; a < 6; ++a )
   {
      HH_REQUIRE( written[a] != muV && written[a] != muE, w + ": a written array must not alias src, mu or another written array" );
      for ( int k = 0; k < 3; ++k )
         HH_REQUIRE( written[a] != srcV[k] && written[a] != srcE[k], w + ": a written array must not alias src, mu or another written array" );
      for ( int b = a + 1; b < 6; ++b )
         HH_REQUIRE( written[a] != written[b], w + ": a written array must not alias src, mu or another written array" );
   }
   HH_REQUIRE( update == HYTEG_HIP_REPLACE || update == HYTEG_HIP_ADD, w + ": bad update type" );
   return HYTEG_HIP_OK;
}

EkArgs make_args( double* const* dstV, double* const* dstE, const double* const* srcV, const double* const* srcE, const double* muV, const double* muE,
                  int level, const double* geometry, double alpha, int update, const unsigned mask[3], unsigned kinds )
{
   EkArgs A{};
   for ( int k = 0; k < 3; ++k )
      A.dstV[k] = dstV[k], A.dstE[k] = dstE[k], A.srcV[k] = srcV[k], A.srcE[k] = srcE[k], A.mask[k] = mask[k];
   A.muV = muV, A.muE = muE, A.alpha = alpha;
   A.N = ( 1 << level ) + 1, A.update = update, A.kinds = kinds;
   for ( int t = 0; t < 6; ++t )
      for ( int p = 0; p < 12; ++p )
         A.W.h[t][p] = geometry[12 * t + p];
   return A;
}

// the gather form on the DoFs of A.mask: all entries of the kinds' arrays if a component asks for an inner DoF, else the boundary walk.
// Eight lanes per DoF where the launch is latency-bound (the boundary walk, and all DoFs up to level 5); one lane per DoF above.
constexpr int kGatherLanes = 8, kGatherLanesMaxLevel = 5;
int launch_gather( const EkArgs& A, int level, hipStream_t s )
{
   EkGatherArgs G;
   G.A = A, G.T = tables();
   if ( ( A.mask[0] | A.mask[1] | A.mask[2] ) & HYTEG_HIP_MASK_INNER )
   {
      const unsigned dofs = tet32( (unsigned) A.N );
      if ( level <= kGatherLanesMaxLevel )
         hipLaunchKernelGGL( ( p2_epsilon_gather_kernel< true, kGatherLanes, false > ), dim3( ( dofs * kGatherLanes + kThreads - 1 ) / kThreads, 8 ),
                             dim3( kThreads ), 0, s, G );
      else
         hipLaunchKernelGGL( ( p2_epsilon_gather_kernel< true, 1, false > ), dim3( ( dofs + kThreads - 1 ) / kThreads, 8 ), dim3( kThreads ), 0, s, G );
   }
   else
   {
      const unsigned dofs = (unsigned) ( 4 * tri( A.N ) );
      hipLaunchKernelGGL( ( p2_epsilon_gather_kernel< false, kGatherLanes, false > ), dim3( ( dofs * kGatherLanes + kThreads - 1 ) / kThreads, 8 ),
                          dim3( kThreads ), 0, s, G );
   }
   HH_CHECK_HIP( hipGetLastError() );
   return HYTEG_HIP_OK;
}

// masks[3] & HYTEG_HIP_MASK_ALL; false if nothing is selected
bool clean_masks( const unsigned* mask, unsigned& kind_mask, unsigned out[3] )
{
   for ( int k = 0; k < 3; ++k )
      out[k] = mask[k] & HYTEG_HIP_MASK_ALL;
   kind_mask &= 0xFFu;
   return ( out[0] | out[1] | out[2] ) != 0 && kind_mask != 0;
}

} // namespace

extern "C" {

HYTEG_HIP_API int hyteg_hip_p2_elementwise_epsilon_geometry( const double* macro_vertex_coords, int level, double* geometry )
{
   const char* who = "p2_elementwise_epsilon_geometry";
   HH_REQUIRE( macro_vertex_coords && geometry, std::string( who ) + ": null pointer" );
   HH_REQUIRE( level >= 0 && level <= kP2EpsilonMaxLevel, std::string( who ) + ": level out of range [0,8]" );
   double cc[4][3];
   for ( int v = 0; v < 4; ++v )
      for ( int r = 0; r < 3; ++r )
         cc[v][r] = macro_vertex_coords[3 * v + r];
   for ( int t = 0; t < 6; ++t )
   {
      double c[4][3], g[4][3];
      elmat::micro_cell_coords( cc, int64_t( 1 ) << level, t, c );
      const double V = elmat::gradients( c, g );
      HH_REQUIRE( V > 0.0 && std::isfinite( V ), std::string( who ) + ": degenerate macro-cell" );
      const double scale = std::sqrt( V / 840.0 );
      for ( int a = 0; a < 4; ++a )
         for ( int r = 0; r < 3; ++r )
            geometry[12 * t + 3 * a + r] = scale * g[a][r];
   }
   return HYTEG_HIP_OK;
}

HYTEG_HIP_API int hyteg_hip_p2_elementwise_epsilon_apply_cell_kinds( double* const*       dst_vertex,
                                                                     double* const*       dst_edge,
                                                                     const double* const* src_vertex,
                                                                     const double* const* src_edge,
                                                                     const double*        mu_vertex,
                                                                     const double*        mu_edge,
                                                                     const unsigned*      mask,
                                                                     int                  level,
                                                                     const double*        geometry,
                                                                     double               alpha,
                                                                     int                  update,
                                                                     unsigned             kind_mask,
                                                                     hyteg_hip_stream_t   stream )
{
   HH_REQUIRE( mask, "p2_elementwise_epsilon_apply_cell: null pointer" );
   const int rc = validate( "p2_elementwise_epsilon_apply_cell", dst_vertex, dst_edge, src_vertex, src_edge, mu_vertex, mu_edge, level, geometry, update );
   if ( rc != HYTEG_HIP_OK )
      return rc;
   unsigned m[3];
   if ( !clean_masks( mask, kind_mask, m ) )
      return HYTEG_HIP_OK;
   EkArgs         A        = make_args( dst_vertex, dst_edge, src_vertex, src_edge, mu_vertex, mu_edge, level, geometry, alpha, update, m, kind_mask );
   const unsigned any      = m[0] | m[1] | m[2];
   const bool     inner    = ( any & HYTEG_HIP_MASK_INNER ) && level >= 2 && level >= inner_min_level().load( std::memory_order_relaxed );
   if ( !inner )
      return launch_gather( A, level, as_stream( stream ) );
   if ( any & HYTEG_HIP_MASK_SHELL )
   {
      EkArgs B = A;
      for ( int k = 0; k < 3; ++k )
         B.mask[k] = m[k] & HYTEG_HIP_MASK_SHELL;
      const int rs = launch_gather( B, level, as_stream( stream ) );
      if ( rs != HYTEG_HIP_OK )
         return rs;
   }
   const unsigned nb = ( tet32( (unsigned) A.N ) + kThreads - 1 ) / kThreads;
   if ( kind_mask & 1u )
      hipLaunchKernelGGL( p2_epsilon_inner_vertex_kernel, dim3( nb ), dim3( kThreads ), 0, as_stream( stream ), A );
   if ( kind_mask & 0xFEu )
      hipLaunchKernelGGL( p2_epsilon_inner_edge_kernel, dim3( nb, 7 ), dim3( kThreads ), 0, as_stream( stream ), A );
   HH_CHECK_HIP( hipGetLastError() );
   return HYTEG_HIP_OK;
}

HYTEG_HIP_API int hyteg_hip_p2_elementwise_epsilon_apply_cell_gather( double* const*       dst_vertex,
                                                                      double* const*       dst_edge,
                                                                      const double* const* src_vertex,
                                                                      const double* const* src_edge,
                                                                      const double*        mu_vertex,
                                                                      const double*        mu_edge,
                                                                      const unsigned*      mask,
                                                                      int                  level,
                                                                      const double*        geometry,
                                                                      double               alpha,
                                                                      int                  update,
                                                                      unsigned             kind_mask,
                                                                      hyteg_hip_stream_t   stream )
{
   HH_REQUIRE( mask, "p2_elementwise_epsilon_apply_cell_gather: null pointer" );
   const int rc =
       validate( "p2_elementwise_epsilon_apply_cell_gather", dst_vertex, dst_edge, src_vertex, src_edge, mu_vertex, mu_edge, level, geometry, update );
   if ( rc != HYTEG_HIP_OK )
      return rc;
   unsigned m[3];
   if ( !clean_masks( mask, kind_mask, m ) )
      return HYTEG_HIP_OK;
   return launch_gather( make_args( dst_vertex, dst_edge, src_vertex, src_edge, mu_vertex, mu_edge, level, geometry, alpha, update, m, kind_mask ), level,
                         as_stream( stream ) );
}

HYTEG_HIP_API int hyteg_hip_p2_elementwise_epsilon_diagonal_cell( double* const*     diag_vertex,
                                                                  double* const*     diag_edge,
                                                                  const double*      mu_vertex,
                                                                  const double*      mu_edge,
                                                                  int                level,
                                                                  const double*      geometry,
                                                                  hyteg_hip_stream_t stream )
{
   const char* who = "p2_elementwise_epsilon_diagonal_cell";
   HH_REQUIRE( diag_vertex && diag_edge && mu_vertex && mu_edge, std::string( who ) + ": null pointer" );
   const double* src[3] = { mu_vertex, mu_vertex, mu_vertex }; // never read
   const double* sre[3] = { mu_edge, mu_edge, mu_edge };
   const int     rc     = validate( who, diag_vertex, diag_edge, src, sre, mu_vertex, mu_edge, level, geometry, HYTEG_HIP_REPLACE );
   if ( rc != HYTEG_HIP_OK )
      return rc;
   const unsigned all[3] = { HYTEG_HIP_MASK_ALL, HYTEG_HIP_MASK_ALL, HYTEG_HIP_MASK_ALL };
   EkGatherArgs   G;
   G.A = make_args( diag_vertex, diag_edge, src, sre, mu_vertex, mu_edge, level, geometry, 1.0, HYTEG_HIP_REPLACE, all, 0xFFu ), G.T = tables();
   const unsigned dofs = tet32( (unsigned) G.A.N );
   hipLaunchKernelGGL( ( p2_epsilon_gather_kernel< true, kGatherLanes, true > ), dim3( ( dofs * kGatherLanes + kThreads - 1 ) / kThreads, 8 ),
                       dim3( kThreads ), 0, as_stream( stream ), G );
   HH_CHECK_HIP( hipGetLastError() );
   return HYTEG_HIP_OK;
}

HYTEG_HIP_API int hyteg_hip_p2_elementwise_epsilon_set_inner_min_level( int level )
{
   const int before = inner_min_level().load();
   inner_min_level().store( level < 2 ? 2 : level );
   return before;
}

HYTEG_HIP_API int hyteg_hip_p2_elementwise_epsilon_max_level( void ) { return kP2EpsilonMaxLevel; }
}
