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
// Forms, as for div-k-grad: p2_epsilon_gather_kernel (a lane group per DoF, micro-cells from P2Tables: boundary DoFs of every level, all
// DoFs of levels 0-1, the three diagonals and, through an entry of its own, every DoF) and p2_epsilon_inner_vertex_kernel / _edge_kernel
// (compile-time micro-cell lists, index polynomials of dk_at).  Every component has a point-class mask of its own: a component whose mask
// excludes a DoF is computed but not stored.  Fixed summation order; no atomics, no LDS, no scratch.  32-bit indices, levels 0 .. 8.
#pragma once

#include "kernels_p2_divkgrad.hpp"

namespace {

constexpr int kP2EpsilonMaxLevel = kP2DivKGradMaxLevel;

struct EkGeometry
{
   double h[6][12]; // sqrt( |e| / 840 ) d_r l_a of micro-cell type t at [3 a + r]
};

struct EkArgs
{
   double*       dstV[3];
   double*       dstE[3];
   const double* srcV[3];
   const double* srcE[3];
   const double* muV;
   const double* muE;
   double        alpha;
   int           N, update;
   unsigned      mask[3], kinds;
   EkGeometry    W;
};
struct EkGatherArgs
{
   EkArgs   A;
   P2Tables T;
};

// row `row` of the three components of A_e u, without the factor alpha.  h: the twelve scaled gradient components of the micro-cell's
// type.  Every loop has constant bounds and is unrolled; with a compile-time row the entries of S that the row does not need are never
// computed.
__device__ __forceinline__ void ek_element_rows( const double* __restrict__ h, const double ( &mu )[10], const double ( &u )[3][10], int row,
                                                 double ( &res )[3] )
{
   double Q[4][4];
   dk_moments( mu, Q );
   double Z[3][4][3];
#pragma unroll
   for ( int j = 0; j < 3; ++j )
   {
      double w[4][4];
      dk_weights( u[j], w );
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
            out[kDkLocal[a][b]] = 4.0 * ( S[a][b] + S[b][a] );
      }
      double v = out[0];
#pragma unroll
      for ( int k = 1; k < 10; ++k )
         v = row == k ? out[k] : v;
      res[i] = v;
   }
}

// ---- gather form: a group of G lanes per DoF, micro-cells from the tables (the sibling of p2_divkgrad_gather_kernel) ------------
// DIAG: component i of every DoF receives the sum of A_e^{ii}[row][row] (src is not read): the row function on the unit vector of
// the DoF in component i alone, once per component.
template < bool ALL, int G, bool DIAG >
__global__ __launch_bounds__( kThreads ) void p2_epsilon_gather_kernel( const EkGatherArgs GA )
{
   const EkArgs& A = GA.A;
   const int     c = blockIdx.y; // destination kind
   const int     N = A.N, n = N - 1;
   const int     W = c == 0 ? N : ( c == 7 ? n - 1 : n );
   if ( W <= 0 || !( ( A.kinds >> c ) & 1u ) )
      return;
   const int lane = threadIdx.x & ( G - 1 );
   const int q    = blockIdx.x * ( kThreads / G ) + (int) threadIdx.x / G;
   int       x, y, z;
   if constexpr ( ALL )
   {
      if ( q >= (int) tet32( (unsigned) W ) )
         return;
      z           = slice_of( W, q );
      const int j = q - slice_start( W, z );
      y           = row_of( W - z, j );
      x           = j - row_start( W - z, y );
   }
   else
   {
      const int T = tri( W );
      if ( q >= 4 * T )
         return;
      const int f = q / T, r = q - f * T;
      const int j = row_of( W, r );
      const int k = r - row_start( W, j );
      switch ( f )
      {
      case 0:
         x = k, y = j, z = 0;
         break;
      case 1:
         x = k, y = 0, z = j;
         break;
      case 2:
         x = 0, y = k, z = j;
         break;
      default:
         x = k, y = j, z = W - 1 - k - j;
         break;
      }
      const int lowest = ( z == 0 ) ? 0 : ( y == 0 ) ? 1 : ( x == 0 ) ? 2 : 3;
      if ( lowest != f )
         return;
   }
   const int cls = c == 0 ? slot_from_flags< 14 >( z == 0, y == 0, x == 0, x + y + z == N - 1 ) : edge_class( N, x, y, z, c - 1 );
   if ( !( ( ( A.mask[0] | A.mask[1] | A.mask[2] ) >> cls ) & 1u ) )
      return;
   // every lane of a DoF's group is still here, or none is
   const int i = cell_index( W, x, y, z );
   // one adjacent micro-cell: alpha * ( the three rows of its element matrix ) . ( its thirty source values )
   auto contribution = [&]( int l, double ( &part )[3] ) -> bool {
      const Entry en = GA.T.entries[c][l];
      const int   t = en.type, mx = x - en.ox, my = y - en.oy, mz = z - en.oz;
      const int   rows = n - kRowDeficit[t];
      if ( mx < 0 || my < 0 || mz < 0 || mx + my + mz > rows - 1 )
         return false; // the micro-cell is not inside the macro-cell; inside, all its ten DoFs are
      double mu[10], u[3][10];
#pragma unroll
      for ( int d = 0; d < 10; ++d )
      {
         const LocalDof ld = GA.T.local[t][d];
         const int      px = mx + ld.ox, py = my + ld.oy, pz = mz + ld.oz;
         const int      at = ld.kind == 0 ? cell_index( N, px, py, pz ) : dk_block_start( n, ld.kind ) + cell_index( ld.kind == 7 ? n - 1 : n, px, py, pz );
         mu[d]             = ld.kind == 0 ? A.muV[at] : A.muE[at];
         if constexpr ( !DIAG )
         {
#pragma unroll
            for ( int j = 0; j < 3; ++j )
               u[j][d] = ld.kind == 0 ? A.srcV[j][at] : A.srcE[j][at];
         }
      }
      if constexpr ( DIAG )
      {
#pragma unroll 1
         for ( int k = 0; k < 3; ++k )
         {
#pragma unroll
            for ( int j = 0; j < 3; ++j )
#pragma unroll
               for ( int d = 0; d < 10; ++d )
                  u[j][d] = ( j == k && d == en.row ) ? 1.0 : 0.0;
            double o[3];
            ek_element_rows( A.W.h[t], mu, u, en.row, o );
            part[0] = k == 0 ? o[0] : part[0];
            part[1] = k == 1 ? o[1] : part[1];
            part[2] = k == 2 ? o[2] : part[2];
         }
      }
      else
      {
         double o[3];
         ek_element_rows( A.W.h[t], mu, u, en.row, o );
#pragma unroll
         for ( int j = 0; j < 3; ++j )
            part[j] = A.alpha * o[j];
      }
      return true;
   };
   double acc[3] = { 0.0, 0.0, 0.0 };
   if constexpr ( G > 1 )
   {
      constexpr int      kSlots = 24 / G;
      double             part[kSlots][3];
      unsigned long long vmask[kSlots];
#pragma unroll
      for ( int k = 0; k < kSlots; ++k )
      {
         part[k][0] = part[k][1] = part[k][2] = 0.0;
         const int  l     = lane + k * G;
         const bool valid = l < GA.T.nentries[c] && contribution( l, part[k] );
         vmask[k]         = __ballot( valid );
      }
      const int base = ( threadIdx.x & 63 ) & ~( G - 1 ); // first lane of this DoF's group inside the wave
#pragma unroll
      for ( int l = 0; l < 24; ++l )
      {
         const bool on = ( vmask[l / G] >> ( base + ( l % G ) ) ) & 1ull;
#pragma unroll
         for ( int j = 0; j < 3; ++j )
         {
            const double p = __shfl( part[l / G][j], base + ( l % G ), 64 );
            if ( on )
               acc[j] += p;
         }
      }
      if ( lane != 0 )
         return;
   }
   else
   {
      for ( int l = 0; l < GA.T.nentries[c]; ++l )
      {
         double part[3] = { 0.0, 0.0, 0.0 };
         if ( contribution( l, part ) )
         {
#pragma unroll
            for ( int j = 0; j < 3; ++j )
               acc[j] += part[j];
         }
      }
   }
   const int at = c == 0 ? i : dk_block_start( n, c ) + i;
#pragma unroll
   for ( int j = 0; j < 3; ++j )
   {
      if ( !( ( A.mask[j] >> cls ) & 1u ) )
         continue;
      double* out = ( c == 0 ? A.dstV[j] : A.dstE[j] ) + at;
      *out        = A.update == HYTEG_HIP_ADD ? *out + acc[j] : acc[j];
   }
}

// ---- inner form: destination kind C, compile-time micro-cell list (dk_cells), the three components in one pass --------------------
// An index as the unsigned 28-bit number it is (the arrays of level 8 have fewer than 2^25 entries): the byte offset then provably fits
// 32 bits, so a load is  scalar base pointer + 32-bit lane offset  and the offset register of a DoF serves all four fields (every load
// of the vertex kernel compiles to that form); a sign-extended index makes every ( array, offset ) pair a 64-bit lane address of its own.
__device__ __forceinline__ unsigned ek_index( int at ) { return (unsigned) at & 0x0FFFFFFFu; }
template < int C, int I >
__device__ __forceinline__ void ek_inner_cell( const EkArgs& A, const DkBase& B, double ( &acc )[3] )
{
   constexpr int T = DkCellsOf< C >::value.type[I], ROW = DkCellsOf< C >::value.row[I];
   constexpr int MX = -DkCellsOf< C >::value.ox[I], MY = -DkCellsOf< C >::value.oy[I], MZ = -DkCellsOf< C >::value.oz[I];
   double        mu[10], u[3][10];
   [&]< int... D >( std::integer_sequence< int, D... > ) {
      const unsigned at[10] = { ek_index( dk_at< DkLocalOf< T, D >::value.kind, MX + DkLocalOf< T, D >::value.ox, MY + DkLocalOf< T, D >::value.oy,
                                                 MZ + DkLocalOf< T, D >::value.oz >( B ) )... };
      ( ( mu[D] = ( DkLocalOf< T, D >::value.kind == 0 ? A.muV : A.muE )[at[D]] ), ... );
      ( ( u[0][D] = ( DkLocalOf< T, D >::value.kind == 0 ? A.srcV[0] : A.srcE[0] )[at[D]] ), ... );
      ( ( u[1][D] = ( DkLocalOf< T, D >::value.kind == 0 ? A.srcV[1] : A.srcE[1] )[at[D]] ), ... );
      ( ( u[2][D] = ( DkLocalOf< T, D >::value.kind == 0 ? A.srcV[2] : A.srcE[2] )[at[D]] ), ... );
   }
   ( std::make_integer_sequence< int, 10 >{} );
   double o[3];
   ek_element_rows( A.W.h[T], mu, u, ROW, o );
#pragma unroll
   for ( int j = 0; j < 3; ++j )
      acc[j] += A.alpha * o[j];
   // one micro-cell at a time: its forty values must not be in flight together with the next cell's
   __builtin_amdgcn_sched_barrier( 0 );
}

template < int C >
__device__ __forceinline__ void ek_inner_body( const EkArgs& A )
{
   constexpr int NC = DkCellsOf< C >::value.n; // forced constant evaluation: none of the table code may run on the device
   const int     N = A.N, n = N - 1;
   const int     W = C == 0 ? N : ( C == 7 ? n - 1 : n );
   const int     q = blockIdx.x * kThreads + (int) threadIdx.x;
   if ( W <= 0 || q >= dk_tet( W ) )
      return;
   const int z = slice_of( W, q );
   const int j = q - ( dk_tet( W ) - dk_tet( W - z ) );
   const int y = row_of( W - z, j );
   const int x = j - row_start( W - z, y );
   if ( !dk_inner< C >( N, x, y, z ) )
      return;
   const DkBase B      = dk_base( N, x, y, z );
   double       acc[3] = { 0.0, 0.0, 0.0 };
   [&]< int... I >( std::integer_sequence< int, I... > ) { ( ek_inner_cell< C, I >( A, B, acc ), ... ); }
   ( std::make_integer_sequence< int, NC >{} );
   // The sums are complete HERE.  Without a use in this block the compiler sinks each component's half of the arithmetic (E, S and the
   // running sum of every cell) into that component's conditional store below and keeps the Z of all cells alive until then: 10 KB of
   // scratch per lane in the vertex kernel.
   asm volatile( "" : "+v"( acc[0] ), "+v"( acc[1] ), "+v"( acc[2] ) );
   const int at = C == 0 ? q : ( C - 1 ) * B.te + q;
#pragma unroll
   for ( int k = 0; k < 3; ++k )
   {
      if ( !( ( A.mask[k] >> 14 ) & 1u ) ) // inner DoFs are point class 14
         continue;
      double* out = ( C == 0 ? A.dstV[k] : A.dstE[k] ) + at;
      *out        = A.update == HYTEG_HIP_ADD ? *out + acc[k] : acc[k];
   }
}

// the inner vertex DoFs (24 micro-cells each) and, blockIdx.y + 1 = destination kind, the inner edge DoFs of the kinds of A.kinds
__global__ __launch_bounds__( kThreads ) void p2_epsilon_inner_vertex_kernel( const EkArgs A ) { ek_inner_body< 0 >( A ); }
__global__ __launch_bounds__( kThreads ) void p2_epsilon_inner_edge_kernel( const EkArgs A )
{
   const int c = blockIdx.y + 1;
   if ( !( ( A.kinds >> c ) & 1u ) )
      return;
   switch ( c )
   {
   case 1:
      ek_inner_body< 1 >( A );
      break;
   case 2:
      ek_inner_body< 2 >( A );
      break;
   case 3:
      ek_inner_body< 3 >( A );
      break;
   case 4:
      ek_inner_body< 4 >( A );
      break;
   case 5:
      ek_inner_body< 5 >( A );
      break;
   case 6:
      ek_inner_body< 6 >( A );
      break;
   default:
      ek_inner_body< 7 >( A );
      break;
   }
}

} // namespace
