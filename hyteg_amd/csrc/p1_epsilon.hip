// C-ABI entry points of the variable-viscosity P1 epsilon operator -div( 2 mu eps(u) ) on one macro-cell: the fused form of the nine
// P1ElementwiseOperator blocks of P1ElementwiseAffineEpsilonOperator (src/mixed_operator/P1EpsilonOperator.hpp:89-164; each
// block: P1ElementwiseOperator::apply, src/hyteg/elementwiseoperators/P1ElementwiseOperator.cpp), of its extractInverseDiagonal
// (the diagonals of the three diagonal blocks), of P1ElementwiseOperator::smooth_jac (P1ElementwiseOperator.cpp:288-331), of the
// residual of a multigrid cycle (GeometricMultigridSolver.hpp:240-246) and of the steps of ChebyshevSmoother::solve
// (ChebyshevSmoother.hpp:165-212) on the three components.  The viscosity is a P1 function: the same operator as the reference's where mu is linear per micro-cell.
// Kernels: kernels_varcoef.hpp with the policy of kernels_epsilon.hpp.
#include "kernels_epsilon.hpp"
#include "varcoef_launch.hpp"

using namespace hyteg_hip;
using namespace hyteg_hip::varcoef;

namespace {

using OpArgs = Args< Epsilon >;

// Brick shape of the z-march: rows x slices per wave.  Four operand arrays are live, so the bricks are smaller than div-k-grad's:
// every compiled shape holds its operands in registers without scratch at one wave per SIMD.  Levels <= 7 are few bricks:
// many short waves; at level 8 two rows per wave load fewer rows twice.  hyteg_hip_p1_elementwise_epsilon_set_shape overrides
// (tests, measurements).
struct Launch
{
   using OP     = Epsilon;
   using Shapes = Bricks< Brick< 1, 4 >, Brick< 1, 8 >, Brick< 2, 4 > >;
   // the Chebyshev step with its second store stream needs scratch at 2 x 4 and is not compiled there: level 8 marches 1 x 8
   template < int MODE, int NY, int LZ >
   static constexpr bool compiled()
   {
      return !( MODE == CHEB_STEP && NY == 2 && LZ == 4 );
   }
   static Shape level_shape( int level, int mode )
   {
      return level <= 7 ? Shape{ 1, 4 } : ( mode == CHEB_STEP ? Shape{ 1, 8 } : Shape{ 2, 4 } );
   }
   static inline Shape shape_override{ 0, 0 };
   // the inner points by the one-thread-per-point kernel instead of the z-march (tests, tools/bench_kernels.py)
   static inline bool inner_by_points = false;
};

inline bool any_null( const double* const* p ) { return !p || !p[0] || !p[1] || !p[2]; }
inline bool among( const double* q, const double* const* p ) { return q == p[0] || q == p[1] || q == p[2]; }

// validation of what every entry shares, and the weights of the six micro-cell types
int prepare( const char* who, const double* coords, int64_t micro_edges, OpArgs& A, int* level )
{
   double    cc[4][3];
   const int rc = prepare_cell( who, coords, micro_edges, cc, A, level );
   if ( rc != HYTEG_HIP_OK )
      return rc;
   for ( int t = 0; t < 6; ++t )
   {
      double c[4][3], g[4][3];
      elmat::micro_cell_coords( cc, micro_edges, t, c );
      const double s = std::sqrt( 0.25 * elmat::gradients( c, g ) );
      for ( int a = 0; a < 4; ++a )
         for ( int r = 0; r < 3; ++r )
            A.W.h[t][a][r] = s * g[a][r];
   }
   return HYTEG_HIP_OK;
}

int apply_impl( const char* who, double* const* dst, const double* const* src, const double* mu, const double* coords, int64_t micro_edges,
                const unsigned* masks, int update, hyteg_hip_stream_t stream )
{
   const std::string w( who );
   HH_REQUIRE( !any_null( dst ) && !any_null( src ) && mu && coords && masks, w + ": null pointer" );
   for ( int c = 0; c < 3; ++c )
      HH_REQUIRE( !among( dst[c], src ) && dst[c] != mu && dst[c] != dst[( c + 1 ) % 3], w + ": a dst must not alias src, mu or another dst" );
   HH_REQUIRE( update == HYTEG_HIP_REPLACE || update == HYTEG_HIP_ADD, w + ": bad update type" );
   for ( int c = 0; c < 3; ++c )
      HH_REQUIRE( ( masks[c] & ~(unsigned) HYTEG_HIP_MASK_ALL ) == 0, w + ": bad mask (15 class bits)" );
   OpArgs A{};
   int  level = 0;
   int  rc    = prepare( who, coords, micro_edges, A, &level );
   if ( rc != HYTEG_HIP_OK )
      return rc;
   A.coef = mu;
   for ( int c = 0; c < 3; ++c )
   {
      A.dst[c] = dst[c], A.src[c] = src[c];
      A.masks[c] = masks[c] & HYTEG_HIP_MASK_SHELL;
      A.comps |= ( masks[c] & HYTEG_HIP_MASK_INNER ) ? ( 1u << c ) : 0u;
   }
   const bool add = update == HYTEG_HIP_ADD;
   if ( A.masks[0] | A.masks[1] | A.masks[2] )
   {
      rc = add ? launch_shell< Epsilon, ADD >( A, as_stream( stream ) ) : launch_shell< Epsilon, REPLACE >( A, as_stream( stream ) );
      if ( rc != HYTEG_HIP_OK )
         return rc;
   }
   return add ? launch_inner< Launch, ADD >( A, level, as_stream( stream ) ) : launch_inner< Launch, REPLACE >( A, level, as_stream( stream ) );
}

} // namespace

extern "C" {

HYTEG_HIP_API int hyteg_hip_p1_elementwise_epsilon_apply_macro_3d_masked( double* const*       dst,
                                                                          const double* const* src,
                                                                          const double*        mu,
                                                                          const double*        macro_vertex_coords,
                                                                          int64_t              micro_edges_per_macro_edge,
                                                                          unsigned             mask,
                                                                          int                  update,
                                                                          hyteg_hip_stream_t   stream )
{
   const unsigned masks[3] = { mask, mask, mask };
   return apply_impl( "p1_elementwise_epsilon_apply_macro_3d", dst, src, mu, macro_vertex_coords, micro_edges_per_macro_edge, masks, update, stream );
}

HYTEG_HIP_API int hyteg_hip_p1_elementwise_epsilon_apply_macro_3d_component_masks( double* const*       dst,
                                                                                   const double* const* src,
                                                                                   const double*        mu,
                                                                                   const double*        macro_vertex_coords,
                                                                                   int64_t              micro_edges_per_macro_edge,
                                                                                   const unsigned*      masks,
                                                                                   int                  update,
                                                                                   hyteg_hip_stream_t   stream )
{
   return apply_impl( "p1_elementwise_epsilon_apply_macro_3d_component_masks", dst, src, mu, macro_vertex_coords, micro_edges_per_macro_edge, masks,
                      update, stream );
}

HYTEG_HIP_API int hyteg_hip_p1_elementwise_epsilon_jacobi_macro_3d( double* const*       dst,
                                                                    const double* const* src,
                                                                    const double* const* rhs,
                                                                    const double* const* inv_diag,
                                                                    const double*        mu,
                                                                    const double*        macro_vertex_coords,
                                                                    int64_t              micro_edges_per_macro_edge,
                                                                    double               omega,
                                                                    hyteg_hip_stream_t   stream )
{
   const char* who = "p1_elementwise_epsilon_jacobi_macro_3d";
   HH_REQUIRE( !any_null( dst ) && !any_null( src ) && !any_null( rhs ) && !any_null( inv_diag ) && mu && macro_vertex_coords,
               std::string( who ) + ": null pointer" );
   for ( int c = 0; c < 3; ++c )
      HH_REQUIRE( !among( dst[c], src ) && !among( dst[c], rhs ) && !among( dst[c], inv_diag ) && dst[c] != mu && dst[c] != dst[( c + 1 ) % 3],
                  std::string( who ) + ": a dst must not alias an input or another dst" );
   OpArgs A{};
   int  level = 0;
   int  rc    = prepare( who, macro_vertex_coords, micro_edges_per_macro_edge, A, &level );
   if ( rc != HYTEG_HIP_OK )
      return rc;
   A.coef = mu, A.omega = omega, A.comps = 7u;
   for ( int c = 0; c < 3; ++c )
      A.dst[c] = dst[c], A.src[c] = src[c], A.rhs[c] = rhs[c], A.invdiag[c] = inv_diag[c];
   return launch_inner< Launch, JACOBI >( A, level, as_stream( stream ) );
}

// the residual of a multigrid cycle (GeometricMultigridSolver.hpp:240-246) and the steps of ChebyshevSmoother::solve
// (ChebyshevSmoother.hpp:165-212) on the three components, each in one launch over the inner points
HYTEG_HIP_API int hyteg_hip_p1_elementwise_epsilon_residual_macro_3d( double* const*       dst,
                                                                      const double* const* src,
                                                                      const double* const* rhs,
                                                                      const double*        mu,
                                                                      const double*        macro_vertex_coords,
                                                                      int64_t              micro_edges_per_macro_edge,
                                                                      unsigned             comps,
                                                                      hyteg_hip_stream_t   stream )
{
   return residual_entry< Launch, false >( "p1_elementwise_epsilon_residual_macro_3d", prepare, dst, src, rhs, nullptr, mu, macro_vertex_coords,
                                           micro_edges_per_macro_edge, comps, as_stream( stream ) );
}

HYTEG_HIP_API int hyteg_hip_p1_elementwise_epsilon_chebyshev_start_macro_3d( double* const*       t_out,
                                                                             const double* const* rhs,
                                                                             const double* const* x,
                                                                             const double* const* inv_diag,
                                                                             const double*        mu,
                                                                             const double*        macro_vertex_coords,
                                                                             int64_t              micro_edges_per_macro_edge,
                                                                             unsigned             comps,
                                                                             hyteg_hip_stream_t   stream )
{
   return residual_entry< Launch, true >( "p1_elementwise_epsilon_chebyshev_start_macro_3d", prepare, t_out, x, rhs, inv_diag, mu, macro_vertex_coords,
                                          micro_edges_per_macro_edge, comps, as_stream( stream ) );
}

HYTEG_HIP_API int hyteg_hip_p1_elementwise_epsilon_chebyshev_step_macro_3d( double* const*       t_out,
                                                                            double* const*       x,
                                                                            const double* const* t_in,
                                                                            const double* const* inv_diag,
                                                                            const double*        mu,
                                                                            const double*        macro_vertex_coords,
                                                                            int64_t              micro_edges_per_macro_edge,
                                                                            double               c_prev,
                                                                            double               c_cur,
                                                                            int                  has_prev,
                                                                            unsigned             comps,
                                                                            hyteg_hip_stream_t   stream )
{
   return chebyshev_step_entry< Launch >( "p1_elementwise_epsilon_chebyshev_step_macro_3d", prepare, t_out, x, t_in, inv_diag, mu, macro_vertex_coords,
                                          micro_edges_per_macro_edge, c_prev, c_cur, has_prev, comps, as_stream( stream ) );
}

HYTEG_HIP_API int hyteg_hip_p1_elementwise_epsilon_diagonal_macro_3d( double* const*     diag,
                                                                      const double*      mu,
                                                                      const double*      macro_vertex_coords,
                                                                      int64_t            micro_edges_per_macro_edge,
                                                                      hyteg_hip_stream_t stream )
{
   const char* who = "p1_elementwise_epsilon_diagonal_macro_3d";
   HH_REQUIRE( !any_null( diag ) && mu && macro_vertex_coords, std::string( who ) + ": null pointer" );
   for ( int c = 0; c < 3; ++c )
      HH_REQUIRE( diag[c] != mu && diag[c] != diag[( c + 1 ) % 3], std::string( who ) + ": a diag must not alias mu or another diag" );
   OpArgs A{};
   int  level = 0;
   int  rc    = prepare( who, macro_vertex_coords, micro_edges_per_macro_edge, A, &level );
   if ( rc != HYTEG_HIP_OK )
      return rc;
   A.coef = mu, A.comps = 7u;
   for ( int c = 0; c < 3; ++c )
      A.dst[c] = diag[c], A.src[c] = mu, A.masks[c] = HYTEG_HIP_MASK_SHELL;
   rc = launch_shell< Epsilon, DIAG >( A, as_stream( stream ) );
   if ( rc != HYTEG_HIP_OK || level < HYTEG_HIP_MIN_LEVEL )
      return rc;
   return launch_inner_points< Epsilon, DIAG >( A, level, as_stream( stream ) );
}

HYTEG_HIP_API int hyteg_hip_p1_elementwise_epsilon_set_shape( int ny, int lz )
{
   return set_shape< Launch >( "p1_elementwise_epsilon_set_shape", ny, lz );
}

HYTEG_HIP_API int hyteg_hip_p1_elementwise_epsilon_set_inner_by_points( int on )
{
   Launch::inner_by_points = on != 0;
   return HYTEG_HIP_OK;
}
}
