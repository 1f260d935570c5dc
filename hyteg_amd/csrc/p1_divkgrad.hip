// C-ABI entry points of the variable-coefficient P1 diffusion operator -div( k grad u ) on one macro-cell: the seam of the generated
// operatorgeneration::P1ElementwiseDivKGrad (apply_macro_3D / computeInverseDiagonalOperatorValues_macro_3D of module
// hyteg_operators; known-answer test tests/hyteg/convergence/ElementwiseDivKGradCGConvergenceTest.cpp) and the fused form of
// P1ElementwiseOperator::smooth_jac (src/hyteg/elementwiseoperators/P1ElementwiseOperator.cpp:288-331), of the residual of a multigrid
// cycle (GeometricMultigridSolver.hpp:240-246) and of the steps of ChebyshevSmoother::solve (ChebyshevSmoother.hpp:165-212).  Kernels: kernels_varcoef.hpp with the policy of kernels_divkgrad.hpp.
#include "kernels_divkgrad.hpp"
#include "varcoef_launch.hpp"

using namespace hyteg_hip;
using namespace hyteg_hip::varcoef;

namespace {

using OpArgs = Args< DivKGrad >;

// Brick shape of the z-march: rows x slices per wave (loads run one slice ahead).  The kernel holds two arrays in registers, so its
// bricks are lower than the constant-stencil kernel's.  Levels <= 7 are a few hundred bricks: many short waves; level 8 marches
// eight slices so that fewer slices are loaded twice.  hyteg_hip_p1_elementwise_divkgrad_set_shape overrides (tests, measurements).
struct Launch
{
   using OP     = DivKGrad;
   using Shapes = Bricks< Brick< 2, 4 >, Brick< 2, 8 >, Brick< 1, 8 > >;
   template < int MODE, int NY, int LZ >
   static constexpr bool compiled()
   {
      return true;
   }
   static Shape level_shape( int level, int /* mode */ ) { return level <= 7 ? Shape{ 2, 4 } : Shape{ 2, 8 }; }
   static inline Shape shape_override{ 0, 0 };
   // measurement switch (tools/bench_kernels.py): the inner points by the one-thread-per-point kernel instead of the z-march
   static inline bool inner_by_points = false;
};

// validation of what every entry shares, and the weights: 0.25 K_t of the six micro-cell types
int prepare( const char* who, const double* coords, int64_t micro_edges, OpArgs& A, int* level )
{
   double    cc[4][3];
   const int rc = prepare_cell( who, coords, micro_edges, cc, A, level );
   if ( rc != HYTEG_HIP_OK )
      return rc;
   for ( int t = 0; t < 6; ++t )
   {
      double c[4][3], Ke[4][4];
      elmat::micro_cell_coords( cc, micro_edges, t, c );
      elmat::p1_diffusion( c, Ke );
      for ( int a = 0; a < 4; ++a )
      {
         A.W.diag[t][a] = 0.25 * Ke[a][a];
         for ( int b = a + 1; b < 4; ++b )
            A.W.off[t][pair_index( a, b )] = 0.25 * Ke[a][b];
      }
   }
   return HYTEG_HIP_OK;
}

} // namespace

extern "C" {

HYTEG_HIP_API int hyteg_hip_p1_elementwise_divkgrad_apply_macro_3d_masked( double*            dst,
                                                                           const double*      src,
                                                                           const double*      k,
                                                                           const double*      macro_vertex_coords,
                                                                           int64_t            micro_edges_per_macro_edge,
                                                                           unsigned           mask,
                                                                           int                update,
                                                                           hyteg_hip_stream_t stream )
{
   const char* who = "p1_elementwise_divkgrad_apply_macro_3d";
   HH_REQUIRE( dst && src && k && macro_vertex_coords, std::string( who ) + ": null pointer" );
   HH_REQUIRE( dst != src && dst != k, std::string( who ) + ": dst must not alias src or k" );
   HH_REQUIRE( update == HYTEG_HIP_REPLACE || update == HYTEG_HIP_ADD, std::string( who ) + ": bad update type" );
   HH_REQUIRE( ( mask & ~(unsigned) HYTEG_HIP_MASK_ALL ) == 0, std::string( who ) + ": bad mask (15 class bits)" );
   OpArgs A{};
   int  level = 0;
   int  rc    = prepare( who, macro_vertex_coords, micro_edges_per_macro_edge, A, &level );
   if ( rc != HYTEG_HIP_OK )
      return rc;
   A.dst[0] = dst, A.src[0] = src, A.coef = k;
   A.masks[0] = mask & HYTEG_HIP_MASK_SHELL;
   A.comps    = ( mask & HYTEG_HIP_MASK_INNER ) ? 1u : 0u;
   const bool add = update == HYTEG_HIP_ADD;
   if ( A.masks[0] )
   {
      rc = add ? launch_shell< DivKGrad, ADD >( A, as_stream( stream ) ) : launch_shell< DivKGrad, REPLACE >( A, as_stream( stream ) );
      if ( rc != HYTEG_HIP_OK )
         return rc;
   }
   return add ? launch_inner< Launch, ADD >( A, level, as_stream( stream ) ) : launch_inner< Launch, REPLACE >( A, level, as_stream( stream ) );
}

HYTEG_HIP_API int hyteg_hip_p1_elementwise_divkgrad_jacobi_macro_3d( double*            dst,
                                                                     const double*      src,
                                                                     const double*      rhs,
                                                                     const double*      inv_diag,
                                                                     const double*      k,
                                                                     const double*      macro_vertex_coords,
                                                                     int64_t            micro_edges_per_macro_edge,
                                                                     double             omega,
                                                                     hyteg_hip_stream_t stream )
{
   const char* who = "p1_elementwise_divkgrad_jacobi_macro_3d";
   HH_REQUIRE( dst && src && rhs && inv_diag && k && macro_vertex_coords, std::string( who ) + ": null pointer" );
   HH_REQUIRE( dst != src && dst != k && dst != rhs && dst != inv_diag, std::string( who ) + ": dst must not alias an input" );
   OpArgs A{};
   int  level = 0;
   int  rc    = prepare( who, macro_vertex_coords, micro_edges_per_macro_edge, A, &level );
   if ( rc != HYTEG_HIP_OK )
      return rc;
   A.dst[0] = dst, A.src[0] = src, A.coef = k, A.rhs[0] = rhs, A.invdiag[0] = inv_diag, A.omega = omega, A.comps = 1u;
   return launch_inner< Launch, JACOBI >( A, level, as_stream( stream ) );
}

// the residual of a multigrid cycle (GeometricMultigridSolver.hpp:240-246) and the steps of ChebyshevSmoother::solve
// (ChebyshevSmoother.hpp:165-212), each in one launch over the inner points
HYTEG_HIP_API int hyteg_hip_p1_elementwise_divkgrad_residual_macro_3d( double*            dst,
                                                                       const double*      src,
                                                                       const double*      rhs,
                                                                       const double*      k,
                                                                       const double*      macro_vertex_coords,
                                                                       int64_t            micro_edges_per_macro_edge,
                                                                       hyteg_hip_stream_t stream )
{
   return residual_entry< Launch, false >( "p1_elementwise_divkgrad_residual_macro_3d", prepare, &dst, &src, &rhs, nullptr, k, macro_vertex_coords,
                                           micro_edges_per_macro_edge, 1u, as_stream( stream ) );
}

HYTEG_HIP_API int hyteg_hip_p1_elementwise_divkgrad_chebyshev_start_macro_3d( double*            t_out,
                                                                              const double*      rhs,
                                                                              const double*      x,
                                                                              const double*      inv_diag,
                                                                              const double*      k,
                                                                              const double*      macro_vertex_coords,
                                                                              int64_t            micro_edges_per_macro_edge,
                                                                              hyteg_hip_stream_t stream )
{
   return residual_entry< Launch, true >( "p1_elementwise_divkgrad_chebyshev_start_macro_3d", prepare, &t_out, &x, &rhs, &inv_diag, k,
                                          macro_vertex_coords, micro_edges_per_macro_edge, 1u, as_stream( stream ) );
}

HYTEG_HIP_API int hyteg_hip_p1_elementwise_divkgrad_chebyshev_step_macro_3d( double*            t_out,
                                                                             double*            x,
                                                                             const double*      t_in,
                                                                             const double*      inv_diag,
                                                                             const double*      k,
                                                                             const double*      macro_vertex_coords,
                                                                             int64_t            micro_edges_per_macro_edge,
                                                                             double             c_prev,
                                                                             double             c_cur,
                                                                             int                has_prev,
                                                                             hyteg_hip_stream_t stream )
{
   return chebyshev_step_entry< Launch >( "p1_elementwise_divkgrad_chebyshev_step_macro_3d", prepare, &t_out, &x, &t_in, &inv_diag, k,
                                          macro_vertex_coords, micro_edges_per_macro_edge, c_prev, c_cur, has_prev, 1u, as_stream( stream ) );
}

HYTEG_HIP_API int hyteg_hip_p1_elementwise_divkgrad_diagonal_macro_3d( double*            diag,
                                                                       const double*      k,
                                                                       const double*      macro_vertex_coords,
                                                                       int64_t            micro_edges_per_macro_edge,
                                                                       hyteg_hip_stream_t stream )
{
   const char* who = "p1_elementwise_divkgrad_diagonal_macro_3d";
   HH_REQUIRE( diag && k && macro_vertex_coords, std::string( who ) + ": null pointer" );
   HH_REQUIRE( diag != k, std::string( who ) + ": diag must not alias k" );
   OpArgs A{};
   int  level = 0;
   int  rc    = prepare( who, macro_vertex_coords, micro_edges_per_macro_edge, A, &level );
   if ( rc != HYTEG_HIP_OK )
      return rc;
   A.dst[0] = diag, A.src[0] = k, A.coef = k, A.masks[0] = HYTEG_HIP_MASK_SHELL, A.comps = 1u;
   rc = launch_shell< DivKGrad, DIAG >( A, as_stream( stream ) );
   if ( rc != HYTEG_HIP_OK || level < HYTEG_HIP_MIN_LEVEL )
      return rc;
   return launch_inner_points< DivKGrad, DIAG >( A, level, as_stream( stream ) );
}

HYTEG_HIP_API int hyteg_hip_p1_elementwise_divkgrad_set_shape( int ny, int lz )
{
   return set_shape< Launch >( "p1_elementwise_divkgrad_set_shape", ny, lz );
}

HYTEG_HIP_API int hyteg_hip_p1_elementwise_divkgrad_set_inner_by_points( int on )
{
   Launch::inner_by_points = on != 0;
   return HYTEG_HIP_OK;
}
}
