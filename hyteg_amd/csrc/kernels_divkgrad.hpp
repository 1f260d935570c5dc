// The variable-coefficient P1 diffusion operator  -div( k grad u )  as an operator policy of kernels_varcoef.hpp (p1_divkgrad.hip).
// Replaces apply_macro_3D and computeInverseDiagonalOperatorValues_macro_3D of the generated
// operatorgeneration::P1ElementwiseDivKGrad (module hyteg_operators; its source is absent from the snapshot, the class is used in
// tests/hyteg/convergence/ElementwiseDivKGradCGConvergenceTest.cpp).  With k linear on a micro-cell e and constant shape-function
// gradients the element matrix is  A_e = mean( k at the 4 vertices of e ) * K_e,  K_e the P1 Laplace element matrix of the
// micro-cell's type (element_matrices.hpp).  K_e has zero row sums, so the value at a point p is
//    sum over the micro-cells e at p:  mean_k( e ) * sum over the three other vertices j of e:  K_e[p, j] * ( u_j - u_p ),
// i.e. 14 differences, one k-sum and three weights per adjacent micro-cell.  The weights depend on ( type, vertex pair ) only:
// 36 wave-uniform doubles in the kernel arguments (with the 1/4 of the mean folded in), never a per-lane table.
#pragma once

#include "kernels_varcoef.hpp"

namespace hyteg_hip {

struct DivKGrad
{
   static constexpr int NC = 1;

   // 0.25 * K_t[a][b], a < b, at varcoef::pair_index( a, b ); the diagonal 0.25 * K_t[a][a] for the point form
   struct Weights
   {
      double off[6][6];
      double diag[6][4];
   };

   // d[0][15]: the differences u_j - u_p to the point's stencil neighbours, k[15]: the coefficient there
   template < int C >
   __device__ static void cell_term( const varcoef::Args< DivKGrad >& A, const double ( &d )[1][15], const double ( &k )[15], double ( &acc )[1] )
   {
      using E        = varcoef::Cell< C >;
      const double m = E::coef_sum( k );
      double       g = A.W.off[E::t][varcoef::pair_index( E::i, E::ja )] * d[0][E::a];
      g              = fma( A.W.off[E::t][varcoef::pair_index( E::i, E::jb )], d[0][E::b], g );
      g              = fma( A.W.off[E::t][varcoef::pair_index( E::i, E::jc )], d[0][E::c], g );
      acc[0] += m * g;
   }

   // m: k summed over the vertices of the type-t micro-cell with the point as local vertex i, d[0][j]: u at vertex j minus u at the point
   template < bool DIAG >
   __device__ static void point_cell( const varcoef::Args< DivKGrad >& A, int t, int i, double m, const double ( &d )[1][4], double ( &acc )[1] )
   {
      double g = 0.0;
      if ( !DIAG )
#pragma unroll
         for ( int j = 0; j < 4; ++j )
            if ( j != i )
               g = fma( A.W.off[t][varcoef::pair_index( i, j )], d[0][j], g );
      acc[0] += DIAG ? m * A.W.diag[t][i] : m * g;
   }
};

} // namespace hyteg_hip
