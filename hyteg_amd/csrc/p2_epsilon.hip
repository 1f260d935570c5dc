// C-ABI entry points of the variable-viscosity P2 epsilon operator -div( 2 mu eps( u ) ) with a P2 viscosity on one macro-cell: the
// seam of operatorgeneration::P2ViscousBlockEpsilonOperator (apply / computeInverseDiagonalOperatorValues; the velocity block of
// operatorgeneration::P2P1StokesEpsilonOperator, whose mu = 1 case is the P2 half of
// tests/hyteg/convergence/ElementwiseEpsilonMinResConvergenceTest.cpp:156-163, 366-412).  Kernels and the arithmetic:
// kernels_p2_epsilon.hpp.
#include "kernels_p2_epsilon.hpp"
#include "p2_varcoef_launch.hpp"

namespace {

struct L
{
   using OP = P2EpsilonOp;
   // first level whose inner DoFs are computed by the inner form (compile-time micro-cell lists); below, and for the boundary DoFs of
   // every level, the gather form.  Measured per level in one run (tools/bench_kernels.py --only p2-epsilon): the inner
   // form is a long dependent chain per thread and loses to the gather form at levels 4 to 6 (73 against 21 us, 78 against 43 us,
   // 139 against 117 us); it wins at level 7 (754 against 832 us), beyond the spread of five repeats.
   static constexpr int         kInnerMinLevelDefault = 7;
   static constexpr const char* kInnerMinLevelEnv     = "HYTEG_HIP_P2_EPSILON_INNER_MIN_LEVEL";
   static constexpr int         kGatherLanes = 8, kGatherLanesMaxLevel = 5;
};

} // namespace

extern "C" {

HYTEG_HIP_API int hyteg_hip_p2_elementwise_epsilon_geometry( const double* macro_vertex_coords, int level, double* geometry )
{
   return p2varcoef::geometry( "p2_elementwise_epsilon_geometry", macro_vertex_coords, level, geometry, [&]( int t, double V, const double( &g )[4][3] ) {
      const double scale = std::sqrt( V / 840.0 );
      for ( int a = 0; a < 4; ++a )
         for ( int r = 0; r < 3; ++r )
            geometry[12 * t + 3 * a + r] = scale * g[a][r];
   } );
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
   return p2varcoef::apply< L >( "p2_elementwise_epsilon_apply_cell", false, dst_vertex, dst_edge, src_vertex, src_edge, mu_vertex, mu_edge, mask, level,
                                 geometry, alpha, update, kind_mask, as_stream( stream ) );
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
   return p2varcoef::apply< L >( "p2_elementwise_epsilon_apply_cell_gather", true, dst_vertex, dst_edge, src_vertex, src_edge, mu_vertex, mu_edge, mask, level,
                                 geometry, alpha, update, kind_mask, as_stream( stream ) );
}

HYTEG_HIP_API int hyteg_hip_p2_elementwise_epsilon_diagonal_cell( double* const*     diag_vertex,
                                                                  double* const*     diag_edge,
                                                                  const double*      mu_vertex,
                                                                  const double*      mu_edge,
                                                                  int                level,
                                                                  const double*      geometry,
                                                                  hyteg_hip_stream_t stream )
{
   return p2varcoef::diagonal< L >( "p2_elementwise_epsilon_diagonal_cell", diag_vertex, diag_edge, mu_vertex, mu_edge, level, geometry, as_stream( stream ) );
}

// The fused modes: the arguments of apply_cell_kinds plus the mode's operands; the _gather entries run the gather form on every DoF.
#define HH_P2_EPSILON_MODE_ENTRIES( SUFFIX, GATHER )                                                                                                   \
   HYTEG_HIP_API int hyteg_hip_p2_elementwise_epsilon_residual_cell##SUFFIX(                                                                           \
       double* const* dst_vertex, double* const* dst_edge, const double* const* src_vertex, const double* const* src_edge,                            \
       const double* const* rhs_vertex, const double* const* rhs_edge, const double* mu_vertex, const double* mu_edge, const unsigned* mask,           \
       int level, const double* geometry, unsigned kind_mask, hyteg_hip_stream_t stream )                                                             \
   {                                                                                                                                                   \
      return p2varcoef::residual< L >( "p2_elementwise_epsilon_residual_cell" #SUFFIX, GATHER, { dst_vertex, dst_edge }, { src_vertex, src_edge },     \
                                       { rhs_vertex, rhs_edge }, mu_vertex, mu_edge, mask, level, geometry, kind_mask, as_stream( stream ) );          \
   }                                                                                                                                                   \
   HYTEG_HIP_API int hyteg_hip_p2_elementwise_epsilon_jacobi_cell##SUFFIX(                                                                             \
       double* const* dst_vertex, double* const* dst_edge, const double* const* src_vertex, const double* const* src_edge,                            \
       const double* const* rhs_vertex, const double* const* rhs_edge, const double* const* invdiag_vertex, const double* const* invdiag_edge,         \
       const double* mu_vertex, const double* mu_edge, const unsigned* mask, int level, const double* geometry, double relax, unsigned kind_mask,      \
       hyteg_hip_stream_t stream )                                                                                                                     \
   {                                                                                                                                                   \
      return p2varcoef::jacobi< L >( "p2_elementwise_epsilon_jacobi_cell" #SUFFIX, GATHER, { dst_vertex, dst_edge }, { src_vertex, src_edge },         \
                                     { rhs_vertex, rhs_edge }, { invdiag_vertex, invdiag_edge }, mu_vertex, mu_edge, mask, level, geometry, relax,     \
                                     kind_mask, as_stream( stream ) );                                                                                 \
   }                                                                                                                                                   \
   HYTEG_HIP_API int hyteg_hip_p2_elementwise_epsilon_chebyshev_start_cell##SUFFIX(                                                                    \
       double* const* t_out_vertex, double* const* t_out_edge, const double* const* x_vertex, const double* const* x_edge,                            \
       const double* const* rhs_vertex, const double* const* rhs_edge, const double* const* invdiag_vertex, const double* const* invdiag_edge,         \
       const double* mu_vertex, const double* mu_edge, const unsigned* mask, int level, const double* geometry, unsigned kind_mask,                    \
       hyteg_hip_stream_t stream )                                                                                                                     \
   {                                                                                                                                                   \
      return p2varcoef::chebyshev_start< L >( "p2_elementwise_epsilon_chebyshev_start_cell" #SUFFIX, GATHER, { t_out_vertex, t_out_edge },             \
                                              { x_vertex, x_edge }, { rhs_vertex, rhs_edge }, { invdiag_vertex, invdiag_edge }, mu_vertex, mu_edge,    \
                                              mask, level, geometry, kind_mask, as_stream( stream ) );                                                 \
   }                                                                                                                                                   \
   HYTEG_HIP_API int hyteg_hip_p2_elementwise_epsilon_chebyshev_step_cell##SUFFIX(                                                                     \
       double* const* t_out_vertex, double* const* t_out_edge, double* const* x_vertex, double* const* x_edge, const double* const* t_in_vertex,      \
       const double* const* t_in_edge, const double* const* invdiag_vertex, const double* const* invdiag_edge, const double* mu_vertex,                \
       const double* mu_edge, const unsigned* mask, int level, const double* geometry, double c_prev, double c_cur, int has_prev,                      \
       unsigned kind_mask, hyteg_hip_stream_t stream )                                                                                                 \
   {                                                                                                                                                   \
      return p2varcoef::chebyshev_step< L >( "p2_elementwise_epsilon_chebyshev_step_cell" #SUFFIX, GATHER, { t_out_vertex, t_out_edge },               \
                                             { x_vertex, x_edge }, { t_in_vertex, t_in_edge }, { invdiag_vertex, invdiag_edge }, mu_vertex, mu_edge,   \
                                             mask, level, geometry, c_prev, c_cur, has_prev, kind_mask, as_stream( stream ) );                         \
   }
HH_P2_EPSILON_MODE_ENTRIES(, false )
HH_P2_EPSILON_MODE_ENTRIES( _gather, true )
#undef HH_P2_EPSILON_MODE_ENTRIES

HYTEG_HIP_API int hyteg_hip_p2_elementwise_epsilon_set_inner_min_level( int level ) { return p2varcoef::set_inner_min_level< L >( level ); }

HYTEG_HIP_API int hyteg_hip_p2_elementwise_epsilon_max_level( void ) { return p2varcoef::kMaxLevel; }
}
