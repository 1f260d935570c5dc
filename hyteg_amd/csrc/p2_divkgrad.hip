// C-ABI entry points of the variable-coefficient P2 diffusion operator -div( k grad u ) with a P2 coefficient on one macro-cell:
// the seam of the generated operatorgeneration::P2ElementwiseDivKGrad (apply / computeInverseDiagonalOperatorValues of module
// hyteg_operators; in-tree use: tests/hyteg/convergence/ElementwiseDivKGradCGConvergenceTest.cpp:192-221).  Kernels and the
// arithmetic: kernels_p2_divkgrad.hpp.
#include "kernels_p2_divkgrad.hpp"
#include "p2_varcoef_launch.hpp"

namespace {

struct L
{
   using OP = P2DivKGradOp;
   // first level whose inner DoFs are computed by the inner form (compile-time micro-cell lists); below, and for the boundary DoFs of
   // every level, the gather form.  Measured per level in one run (tools/bench_kernels.py --only p2-divkgrad): the inner
   // form is a long dependent chain per thread and loses to the eight-lane gather form at levels 4 and 5 (45 against 18 us, 48 against
   // 26 us); it wins from level 6 (71 against 80 us, 310 against 412 us at level 7), beyond the spread of five repeats.
   static constexpr int         kInnerMinLevelDefault = 6;
   static constexpr const char* kInnerMinLevelEnv     = "HYTEG_HIP_P2_DIVKGRAD_INNER_MIN_LEVEL";
   static constexpr int         kGatherLanes = 8, kGatherLanesMaxLevel = 5;
};

} // namespace

extern "C" {

HYTEG_HIP_API int hyteg_hip_p2_elementwise_divkgrad_geometry( const double* macro_vertex_coords, int level, double* geometry )
{
   return p2varcoef::geometry( "p2_elementwise_divkgrad_geometry", macro_vertex_coords, level, geometry, [&]( int t, double V, const double( &g )[4][3] ) {
      for ( int a = 0; a < 4; ++a )
         for ( int b = a; b < 4; ++b )
            geometry[10 * t + kDkPair[a][b]] = V * ( g[a][0] * g[b][0] + g[a][1] * g[b][1] + g[a][2] * g[b][2] ) / 840.0;
   } );
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
   return p2varcoef::apply< L >( "p2_elementwise_divkgrad_apply_cell", false, &dst_vertex, &dst_edge, &src_vertex, &src_edge, k_vertex, k_edge, &mask, level,
                                 geometry, alpha, update, kind_mask, as_stream( stream ) );
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
   return p2varcoef::apply< L >( "p2_elementwise_divkgrad_apply_cell_gather", true, &dst_vertex, &dst_edge, &src_vertex, &src_edge, k_vertex, k_edge, &mask,
                                 level, geometry, alpha, update, kind_mask, as_stream( stream ) );
}

HYTEG_HIP_API int hyteg_hip_p2_elementwise_divkgrad_diagonal_cell( double*            diag_vertex,
                                                                   double*            diag_edge,
                                                                   const double*      k_vertex,
                                                                   const double*      k_edge,
                                                                   int                level,
                                                                   const double*      geometry,
                                                                   hyteg_hip_stream_t stream )
{
   return p2varcoef::diagonal< L >( "p2_elementwise_divkgrad_diagonal_cell", &diag_vertex, &diag_edge, k_vertex, k_edge, level, geometry, as_stream( stream ) );
}

// The fused modes: the arguments of apply_cell_kinds plus the mode's operands; the _gather entries run the gather form on every DoF.
#define HH_P2_DIVKGRAD_MODE_ENTRIES( SUFFIX, GATHER )                                                                                                  \
   HYTEG_HIP_API int hyteg_hip_p2_elementwise_divkgrad_residual_cell##SUFFIX(                                                                          \
       double* dst_vertex, double* dst_edge, const double* src_vertex, const double* src_edge, const double* rhs_vertex, const double* rhs_edge,       \
       const double* k_vertex, const double* k_edge, int level, const double* geometry, unsigned mask, unsigned kind_mask,                             \
       hyteg_hip_stream_t stream )                                                                                                                     \
   {                                                                                                                                                   \
      return p2varcoef::residual< L >( "p2_elementwise_divkgrad_residual_cell" #SUFFIX, GATHER, { &dst_vertex, &dst_edge },                            \
                                       { &src_vertex, &src_edge }, { &rhs_vertex, &rhs_edge }, k_vertex, k_edge, &mask, level, geometry, kind_mask,    \
                                       as_stream( stream ) );                                                                                          \
   }                                                                                                                                                   \
   HYTEG_HIP_API int hyteg_hip_p2_elementwise_divkgrad_jacobi_cell##SUFFIX(                                                                            \
       double* dst_vertex, double* dst_edge, const double* src_vertex, const double* src_edge, const double* rhs_vertex, const double* rhs_edge,       \
       const double* invdiag_vertex, const double* invdiag_edge, const double* k_vertex, const double* k_edge, int level, const double* geometry,      \
       double relax, unsigned mask, unsigned kind_mask, hyteg_hip_stream_t stream )                                                                    \
   {                                                                                                                                                   \
      return p2varcoef::jacobi< L >( "p2_elementwise_divkgrad_jacobi_cell" #SUFFIX, GATHER, { &dst_vertex, &dst_edge }, { &src_vertex, &src_edge },    \
                                     { &rhs_vertex, &rhs_edge }, { &invdiag_vertex, &invdiag_edge }, k_vertex, k_edge, &mask, level, geometry, relax,  \
                                     kind_mask, as_stream( stream ) );                                                                                 \
   }                                                                                                                                                   \
   HYTEG_HIP_API int hyteg_hip_p2_elementwise_divkgrad_chebyshev_start_cell##SUFFIX(                                                                   \
       double* t_out_vertex, double* t_out_edge, const double* x_vertex, const double* x_edge, const double* rhs_vertex, const double* rhs_edge,       \
       const double* invdiag_vertex, const double* invdiag_edge, const double* k_vertex, const double* k_edge, int level, const double* geometry,      \
       unsigned mask, unsigned kind_mask, hyteg_hip_stream_t stream )                                                                                  \
   {                                                                                                                                                   \
      return p2varcoef::chebyshev_start< L >( "p2_elementwise_divkgrad_chebyshev_start_cell" #SUFFIX, GATHER, { &t_out_vertex, &t_out_edge },          \
                                              { &x_vertex, &x_edge }, { &rhs_vertex, &rhs_edge }, { &invdiag_vertex, &invdiag_edge }, k_vertex,        \
                                              k_edge, &mask, level, geometry, kind_mask, as_stream( stream ) );                                        \
   }                                                                                                                                                   \
   HYTEG_HIP_API int hyteg_hip_p2_elementwise_divkgrad_chebyshev_step_cell##SUFFIX(                                                                    \
       double* t_out_vertex, double* t_out_edge, double* x_vertex, double* x_edge, const double* t_in_vertex, const double* t_in_edge,                 \
       const double* invdiag_vertex, const double* invdiag_edge, const double* k_vertex, const double* k_edge, int level, const double* geometry,      \
       double c_prev, double c_cur, int has_prev, unsigned mask, unsigned kind_mask, hyteg_hip_stream_t stream )                                       \
   {                                                                                                                                                   \
      return p2varcoef::chebyshev_step< L >( "p2_elementwise_divkgrad_chebyshev_step_cell" #SUFFIX, GATHER, { &t_out_vertex, &t_out_edge },            \
                                             { &x_vertex, &x_edge }, { &t_in_vertex, &t_in_edge }, { &invdiag_vertex, &invdiag_edge }, k_vertex,       \
                                             k_edge, &mask, level, geometry, c_prev, c_cur, has_prev, kind_mask, as_stream( stream ) );                \
   }
HH_P2_DIVKGRAD_MODE_ENTRIES(, false )
HH_P2_DIVKGRAD_MODE_ENTRIES( _gather, true )
#undef HH_P2_DIVKGRAD_MODE_ENTRIES

HYTEG_HIP_API int hyteg_hip_p2_elementwise_divkgrad_set_inner_min_level( int level ) { return p2varcoef::set_inner_min_level< L >( level ); }

HYTEG_HIP_API int hyteg_hip_p2_elementwise_divkgrad_max_level( void ) { return p2varcoef::kMaxLevel; }
}
