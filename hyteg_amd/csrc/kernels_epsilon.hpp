// The variable-viscosity P1 epsilon operator  -div( 2 mu eps(u) ),  eps(u) = ( grad u + grad u^T ) / 2,  as an operator policy of
// kernels_varcoef.hpp (p1_epsilon.hip).  Replaces the nine P1ElementwiseOperator blocks of P1ElementwiseAffineEpsilonOperator
// (src/mixed_operator/P1EpsilonOperator.hpp:89-164) by one pass over u, v, w and mu.
// With mu linear on a micro-cell e and constant barycentric gradients g_a the block for test component i, trial component j is
//    A_e^{ij}[a][b] = mean( mu at the 4 vertices of e ) * |e| * ( delta_ij g_a . g_b + g_a[j] g_b[i] ).
// Every block has zero row sums ( sum_b g_b = 0 ), so the value at a point p = local vertex a of e needs only the differences
// d^j_b = u^j_b - u^j_p.  The wave-uniform weights are the scaled gradients h_a = sqrt( |e| / 4 ) g_a, 6 x 4 x 3 doubles in the kernel
// arguments.  Per micro-cell
//    D[j][r] = sum_b h_b[r] d^j_b   ( = sqrt( |e| / 4 ) d_r u^j ),   out_i += musum * sum_r h_a[r] ( D[i][r] + D[r][i] ):
// each adjacent micro-cell's mu-sum is formed once for the three destination components.
#pragma once

#include "kernels_varcoef.hpp"

namespace hyteg_hip {

struct Epsilon
{
   static constexpr int NC = 3;

   // h[t][a][r] = sqrt( |e_t| / 4 ) * d_r ( barycentric function a of the type-t micro-cell )
   struct Weights
   {
      double h[6][4][3];
   };

   // d[j][15]: the differences of component j to the point's stencil neighbours, k[15]: mu there
   template < int C >
   __device__ static void cell_term( const varcoef::Args< Epsilon >& A, const double ( &d )[3][15], const double ( &k )[15], double ( &acc )[3] )
   {
      using E                  = varcoef::Cell< C >;
      const double m           = E::coef_sum( k );
      const double( &h )[4][3] = A.W.h[E::t];
      double D[3][3];
#pragma unroll
      for ( int j = 0; j < 3; ++j )
#pragma unroll
         for ( int r = 0; r < 3; ++r )
            D[j][r] = fma( h[E::jc][r], d[j][E::c], fma( h[E::jb][r], d[j][E::b], h[E::ja][r] * d[j][E::a] ) );
#pragma unroll
      for ( int ic = 0; ic < 3; ++ic )
      {
         double s = h[E::i][0] * ( D[ic][0] + D[0][ic] );
         s        = fma( h[E::i][1], D[ic][1] + D[1][ic], s );
         s        = fma( h[E::i][2], D[ic][2] + D[2][ic], s );
         acc[ic]  = fma( m, s, acc[ic] );
      }
   }

   // m: mu summed over the vertices of the type-t micro-cell with the point as local vertex i, d[c][j]: component c at vertex j minus
   // its value at the point.  DIAG: the diagonal entries of the three diagonal blocks, m * ( |h_i|^2 + h_i[c]^2 ).
   template < bool DIAG >
   __device__ static void point_cell( const varcoef::Args< Epsilon >& A, int t, int i, double m, const double ( &d )[3][4], double ( &acc )[3] )
   {
      const double( &h )[4][3] = A.W.h[t];
      double D[3][3]           = {};
      if ( !DIAG )
#pragma unroll
         for ( int j = 0; j < 4; ++j )
            if ( j != i )
#pragma unroll
               for ( int c = 0; c < 3; ++c )
#pragma unroll
                  for ( int r = 0; r < 3; ++r )
                     D[c][r] = fma( h[j][r], d[c][j], D[c][r] );
      const double hh = h[i][0] * h[i][0] + h[i][1] * h[i][1] + h[i][2] * h[i][2];
#pragma unroll
      for ( int c = 0; c < 3; ++c )
      {
         double s;
         if ( DIAG )
            s = hh + h[i][c] * h[i][c];
         else
         {
            s = h[i][0] * ( D[c][0] + D[0][c] );
            s = fma( h[i][1], D[c][1] + D[1][c], s );
            s = fma( h[i][2], D[c][2] + D[2][c], s );
         }
         acc[c] = fma( m, s, acc[c] );
      }
   }
};

} // namespace hyteg_hip
