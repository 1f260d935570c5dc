// Kernels of the variable-viscosity P2 epsilon operator -div( 2 mu eps( u ) ), eps( u ) = ( grad u + grad u^T ) / 2, with a P2 viscosity
// on one macro-cell: the nine blocks of operatorgeneration::P2ViscousBlockEpsilonOperator (the velocity block of
// operatorgeneration::P2P1StokesEpsilonOperator; in-tree counterpart for mu = 1: P2ElementwiseAffineEpsilonOperator of
// tests/hyteg/convergence/ElementwiseEpsilonMinResConvergenceTest.cpp:156-163) in ONE pass over the three velocity components.
//
// Element matrix.  Weak form  int mu ( grad u + grad u^T ) : grad v;  for the test function phi e_i the integrand is
// mu sum_r ( d_r u^i + d_i u^r ) d_r phi, of degree 4 on a micro-cell e and integrated exactly.  In the notation of
// kernels_p2_divkgrad.hpp ( K, Q_cd = int_e mu l_c l_d, w^j_bd from the ten values of component j, grad phi_a = ( 4 l_a - 1 ) g_a,
// grad phi_ab = 4 ( l_a g_b + l_b g_a ) ):
//    Y^j_bc   = sum_d w^j_bd Q_cd
//    Z^j_c[r] = sum_b g_b[r] Y^j_bc                = int_e mu l_c d_r u^j
//    E^i_c[r] = Z^i_c[r] + Z^r_c[i]
//    S^i_ac   = sum_r g_a[r] E^i_c[r]
//    ( A_e u )^i_a = 4 S^i_aa - sum_c S^i_ac,      ( A_e u )^i_ab = 4 ( S^i_ab + S^i_ba ).
// Q is formed once for the three destination components.  The geometry is the twelve gradient components of each of the six micro-cell
// types, scaled as h_a = sqrt( |e| / 840 ) g_a so that Q stays in its integer-combination form: 72 doubles per ( macro-cell, level ) in
// the kernel arguments.  The diagonal blocks sum to four times the div-k-grad element matrix with k = mu; rigid motions are annihilated.
//
// The kernels, shared with the P2 div-k-grad operator: kernels_p2_varcoef.hpp (moments and weights there).  This file is the operator's
// policy: its geometry numbers and the three rows of its element matrix.
#pragma once

#include "kernels_p2_varcoef.hpp"

namespace {

struct P2EpsilonOp
{
   static constexpr int NC = 3;
   struct Geometry
   {
      double h[6][12]; // sqrt( |e| / 840 ) d_r l_a of micro-cell type t at [3 a + r]
   };
   // the inner kernels index their loads with the 28-bit unsigned form of the index (inner_cell of kernels_p2_varcoef.hpp)
   __device__ static unsigned index( int at ) { return (unsigned) at & 0x0FFFFFFFu; }

   // row `row` of the three components of A_e u, without the factor alpha, on a micro-cell of type t.  Every loop has constant bounds and
   // is unrolled; with a compile-time row the entries of S that the row does not need are never computed.
   __device__ __forceinline__ static void element_rows( const Geometry& W, int t, const double ( &mu )[10], const double ( &u )[3][10], int row,
                                                        double ( &res )[3] )
   {
      const double* __restrict__ h = W.h[t];
      double                     Q[4][4];
      p2varcoef::moments( mu, Q );
      double Z[3][4][3];
#pragma unroll
      for ( int j = 0; j < 3; ++j )
      {
         double w[4][4];
         p2varcoef::weights( u[j], w );
#pragma unroll
         for ( int c = 0; c < 4; ++c )
         {
            double Y[4];
#pragma unroll
            for ( int b = 0; b < 4; ++b )
               Y[b] = ( w[b][0] * Q[c][0] + w[b][1] * Q[c][1] ) + ( w[b][2] * Q[c][2] + w[b][3] * Q[c][3] );
#pragma unroll
            for ( int r = 0; r < 3; ++r )
               Z[j][c][r] = ( h[r] * Y[0] + h[3 + r] * Y[1] ) + ( h[6 + r] * Y[2] + h[9 + r] * Y[3] );
         }
      }
#pragma unroll
      for ( int i = 0; i < 3; ++i )
      {
         double S[4][4];
#pragma unroll
         for ( int c = 0; c < 4; ++c )
         {
            double E[3];
#pragma unroll
            for ( int r = 0; r < 3; ++r )
               E[r] = Z[i][c][r] + Z[r][c][i];
#pragma unroll
            for ( int a = 0; a < 4; ++a )
               S[a][c] = ( h[3 * a] * E[0] + h[3 * a + 1] * E[1] ) + h[3 * a + 2] * E[2];
         }
         double out[10];
#pragma unroll
         for ( int a = 0; a < 4; ++a )
         {
            out[a] = 4.0 * S[a][a] - ( ( S[a][0] + S[a][1] ) + ( S[a][2] + S[a][3] ) );
#pragma unroll
            for ( int b = a + 1; b < 4; ++b )
               out[p2varcoef::kLocal[a][b]] = 4.0 * ( S[a][b] + S[b][a] );
         }
         double v = out[0];
#pragma unroll
         for ( int k = 1; k < 10; ++k )
            v = row == k ? out[k] : v;
         res[i] = v;
      }
   }
};

} // namespace
