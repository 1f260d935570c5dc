// Kernels of the variable-coefficient P2 diffusion operator -div( k grad u ) with a P2 coefficient on one macro-cell
// (operatorgeneration::P2ElementwiseDivKGrad; in-tree use: tests/hyteg/convergence/ElementwiseDivKGradCGConvergenceTest.cpp:192-221).
//
// Element matrix.  On a micro-cell e with barycentric functions l_a, constant gradients g_a and volume |e|, write every factor of the
// integrand  k grad phi_i . grad u  as a HOMOGENEOUS polynomial in l (1 = sum l):
//    k       = sum_ef K_ef l_e l_f          K_aa = k_a,  K_ab = 2 k_ab - ( k_a + k_b ) / 2                     (symmetric, 4 x 4)
//    grad u  = sum_b ( sum_d w_bd l_d ) g_b  w_bb = 3 u_b,  w_bd = 4 u_bd - u_b
//    grad phi_a  = ( 4 l_a - 1 ) g_a = ( 3 l_a - sum_{c != a} l_c ) g_a,      grad phi_ab = 4 ( l_a g_b + l_b g_a )
// The moments Q_cd = int_e k l_c l_d follow from  int_e l^alpha = |e| alpha! / 840  ( |alpha| = 4 ): summing the products of
// Kronecker deltas over the 24 permutations of the four indices gives, with s = sum K, tr = trace K, r_c = sum_f K_cf,
//    840 Q_cd / |e| = s + tr + 2 ( r_c + r_d ) + 2 ( K_cd + K_cc + K_dd ) + delta_cd ( s + tr + 4 r_c + 6 K_cc ).
// Then  Y_bc = sum_d w_bd Q_cd,  S_ac = sum_b ( g_a . g_b ) Y_bc,  and
//    ( A_e u )_a = 4 S_aa - sum_c S_ac,      ( A_e u )_ab = 4 ( S_ab + S_ba ).
// The geometry enters through the ten numbers |e| g_a . g_b / 840 of each of the six micro-cell types: 60 doubles per
// ( macro-cell, level ) in the kernel arguments, read with scalar loads; nothing else depends on the cell.  The arithmetic is exact
// integration of the degree-4 integrand; rows sum to zero and k = 1 gives the P2 Laplace element matrix.
//
// The kernels, shared with the P2 epsilon operator: kernels_p2_varcoef.hpp.  This file is the operator's policy: its geometry numbers
// and the row of its element matrix.
#pragma once

#include "kernels_p2_varcoef.hpp"

namespace {

constexpr int kDkPair[4][4] = { { 0, 1, 2, 3 }, { 1, 4, 5, 6 }, { 2, 5, 7, 8 }, { 3, 6, 8, 9 } };

struct P2DivKGradOp
{
   static constexpr int NC = 1;
   struct Geometry
   {
      double g[6][10]; // |e| g_a . g_b / 840 of micro-cell type t, pairs ( a <= b ) in the order 00 01 02 03 11 12 13 22 23 33
   };
   // the inner kernels index their loads with the signed index as computed
   __device__ static int index( int at ) { return at; }

   // row `row` of A_e times u, without the factor alpha, on a micro-cell of type t.  Every loop has constant bounds and is unrolled;
   // with a compile-time row the entries of S that the row does not need are never computed.
   __device__ __forceinline__ static void element_rows( const Geometry& W, int t, const double ( &k )[10], const double ( &u )[1][10], int row,
                                                        double ( &res )[1] )
   {
      const double* __restrict__ g = W.g[t];
      double                     Q[4][4], w[4][4];
      p2varcoef::moments( k, Q );
      p2varcoef::weights( u[0], w );
      double S[4][4];
#pragma unroll
      for ( int c = 0; c < 4; ++c )
      {
         double Y[4];
#pragma unroll
         for ( int b = 0; b < 4; ++b )
            Y[b] = ( w[b][0] * Q[c][0] + w[b][1] * Q[c][1] ) + ( w[b][2] * Q[c][2] + w[b][3] * Q[c][3] );
#pragma unroll
         for ( int a = 0; a < 4; ++a )
            S[a][c] = ( g[kDkPair[a][0]] * Y[0] + g[kDkPair[a][1]] * Y[1] ) + ( g[kDkPair[a][2]] * Y[2] + g[kDkPair[a][3]] * Y[3] );
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
      for ( int i = 1; i < 10; ++i )
         v = row == i ? out[i] : v;
      res[0] = v;
   }
};

} // namespace
