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
// Two forms.  p2_divkgrad_gather_kernel: the sibling of p2_elementwise_kernel (kernels_p2_gather.hpp), a lane group per DoF, the
// adjacent micro-cells from P2Tables with the inside test: every level's boundary DoFs, all DoFs of levels 0-1, the diagonal, and --
// through an entry of its own -- every DoF (the second implementation).  p2_divkgrad_inner_vertex_kernel / _edge_kernel: the inner DoFs from level 2, the
// destination kind a template parameter and the adjacent micro-cells (24 of a vertex DoF, 4-6 of an edge DoF) with the offsets of
// their ten DoFs a compile-time list, so a thread is straight-line code whose lanes run along x.  Both add the micro-cells'
// contributions in a fixed order; no atomics, no LDS, no scratch.  32-bit indices: levels 0 .. kP2DivKGradMaxLevel.
#pragma once

#include "kernels_p2_gather.hpp"

namespace {

constexpr int kP2DivKGradMaxLevel = 8; // 6 tet( 256 ) + tet( 255 ) entries: far below 2^31

struct DkGeometry
{
   double g[6][10]; // |e| g_a . g_b / 840 of micro-cell type t, pairs ( a <= b ) in the order 00 01 02 03 11 12 13 22 23 33
};

struct DkArgs
{
   double*       dstV;
   double*       dstE;
   const double* srcV;
   const double* srcE;
   const double* kV;
   const double* kE;
   double        alpha;
   int           N, update;
   int           diag; // 1: every DoF receives the sum of A_e[i][i] (src is not read)
   unsigned      mask, kinds;
   DkGeometry    W;
};
struct DkGatherArgs
{
   DkArgs   A;
   P2Tables T;
};

constexpr int kDkPair[4][4]  = { { 0, 1, 2, 3 }, { 1, 4, 5, 6 }, { 2, 5, 7, 8 }, { 3, 6, 8, 9 } };
constexpr int kDkLocal[4][4] = { { 0, 9, 8, 7 }, { 9, 1, 6, 5 }, { 8, 6, 2, 4 }, { 7, 5, 4, 3 } }; // fenics::P2DoFMap

// 840 Q_cd / |e| from the ten coefficient values of a micro-cell (shared with the P2 epsilon kernels, kernels_p2_epsilon.hpp)
__device__ __forceinline__ void dk_moments( const double ( &k )[10], double ( &Q )[4][4] )
{
   double K[4][4], r[4];
#pragma unroll
   for ( int a = 0; a < 4; ++a )
   {
      K[a][a] = k[a];
#pragma unroll
      for ( int b = a + 1; b < 4; ++b )
         K[a][b] = K[b][a] = 2.0 * k[kDkLocal[a][b]] - 0.5 * ( k[a] + k[b] );
   }
   double s = 0.0, tr = 0.0;
#pragma unroll
   for ( int a = 0; a < 4; ++a )
   {
      r[a] = ( K[a][0] + K[a][1] ) + ( K[a][2] + K[a][3] );
      s += r[a];
      tr += K[a][a];
   }
   const double st = s + tr;
#pragma unroll
   for ( int c = 0; c < 4; ++c )
   {
      Q[c][c] = 2.0 * st + 8.0 * r[c] + 12.0 * K[c][c];
#pragma unroll
      for ( int d = c + 1; d < 4; ++d )
         Q[c][d] = Q[d][c] = st + 2.0 * ( r[c] + r[d] ) + 2.0 * ( K[c][d] + ( K[c][c] + K[d][d] ) );
   }
}
// grad u = sum_b ( sum_d w_bd l_d ) g_b from the ten values of u
__device__ __forceinline__ void dk_weights( const double ( &u )[10], double ( &w )[4][4] )
{
#pragma unroll
   for ( int b = 0; b < 4; ++b )
#pragma unroll
      for ( int d = 0; d < 4; ++d )
         w[b][d] = b == d ? 3.0 * u[b] : 4.0 * u[kDkLocal[b][d]] - u[b];
}

// row `row` of A_e times u, without the factor alpha.  g: the ten geometry numbers of the micro-cell's type.  Every loop has
// constant bounds and is unrolled; with a compile-time row the entries of S that the row does not need are never computed.
__device__ __forceinline__ double dk_element_row( const double* __restrict__ g, const double ( &k )[10], const double ( &u )[10], int row )
{
   double Q[4][4], w[4][4];
   dk_moments( k, Q );
   dk_weights( u, w );
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
         out[kDkLocal[a][b]] = 4.0 * ( S[a][b] + S[b][a] );
   }
   double res = out[0];
#pragma unroll
   for ( int i = 1; i < 10; ++i )
      res = row == i ? out[i] : res;
   return res;
}

__device__ inline int dk_block_start( int n, int kind ) { return ( kind - 1 ) * (int) tet32( (unsigned) n ); }

// ---- gather form: a group of G lanes per DoF, micro-cells from the tables ------------------------------------------------------
// ALL: group q is entry q of the kind's array; otherwise the boundary DoFs only, enumerated over the four faces of the kind's
// array as in p2_elementwise_kernel (a point is kept at its lowest-numbered face).  As there, the G lanes of a DoF share its (at
// most 24) adjacent micro-cells, 24 / G each, and every lane then adds all contributions in the order of the table: one lane per DoF
// walks 24 dependent round trips (pure latency below level 7), G = 8 keeps three.
template < bool ALL, int G >
__global__ __launch_bounds__( kThreads ) void p2_divkgrad_gather_kernel( const DkGatherArgs GA )
{
   const DkArgs& A = GA.A;
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
   if ( !( ( A.mask >> cls ) & 1u ) )
      return;
   // every lane of a DoF's group is still here, or none is
   const int i = cell_index( W, x, y, z );
   // one adjacent micro-cell: alpha * ( row of its element matrix ) . ( its ten source values )
   auto contribution = [&]( int l, double& part ) -> bool {
      const Entry en = GA.T.entries[c][l];
      const int   t = en.type, mx = x - en.ox, my = y - en.oy, mz = z - en.oz;
      const int   rows = n - kRowDeficit[t];
      if ( mx < 0 || my < 0 || mz < 0 || mx + my + mz > rows - 1 )
         return false; // the micro-cell is not inside the macro-cell; inside, all its ten DoFs are
      double k[10], u[10];
#pragma unroll
      for ( int d = 0; d < 10; ++d )
      {
         const LocalDof ld = GA.T.local[t][d];
         const int      px = mx + ld.ox, py = my + ld.oy, pz = mz + ld.oz;
         const int      at = ld.kind == 0 ? cell_index( N, px, py, pz ) : dk_block_start( n, ld.kind ) + cell_index( ld.kind == 7 ? n - 1 : n, px, py, pz );
         k[d]              = ld.kind == 0 ? A.kV[at] : A.kE[at];
         u[d]              = A.diag ? ( d == en.row ? 1.0 : 0.0 ) : ( ld.kind == 0 ? A.srcV[at] : A.srcE[at] );
      }
      part = A.alpha * dk_element_row( A.W.g[t], k, u, en.row );
      return true;
   };
   double acc = 0.0;
   if constexpr ( G > 1 )
   {
      constexpr int      kSlots = 24 / G;
      double             part[kSlots];
      unsigned long long vmask[kSlots];
#pragma unroll
      for ( int k = 0; k < kSlots; ++k )
      {
         part[k]          = 0.0;
         const int  l     = lane + k * G;
         const bool valid = l < GA.T.nentries[c] && contribution( l, part[k] );
         vmask[k]         = __ballot( valid );
      }
      const int base = ( threadIdx.x & 63 ) & ~( G - 1 ); // first lane of this DoF's group inside the wave
#pragma unroll
      for ( int l = 0; l < 24; ++l )
      {
         const double p = __shfl( part[l / G], base + ( l % G ), 64 );
         if ( ( vmask[l / G] >> ( base + ( l % G ) ) ) & 1ull )
            acc += p;
      }
      if ( lane != 0 )
         return;
   }
   else
   {
      for ( int l = 0; l < GA.T.nentries[c]; ++l )
      {
         double part;
         if ( contribution( l, part ) )
            acc += part;
      }
   }
   double* out = c == 0 ? A.dstV + i : A.dstE + dk_block_start( n, c ) + i;
   *out        = A.update == HYTEG_HIP_ADD ? *out + acc : acc;
}

// ---- inner form: destination kind C, compile-time micro-cell list -------------------------------------------------------------
struct DkCellList
{
   int n;
   int type[24], row[24], ox[24], oy[24], oz[24];
};
// the micro-cells ( type, base = dof - offset ) that hold a DoF of kind c as their local DoF `row`, in the order ( type, row )
constexpr DkCellList dk_cells( int c )
{
   DkCellList L{};
   for ( int t = 0; t < 6; ++t )
      for ( int k = 0; k < 10; ++k )
      {
         const CLocal l = c_local( t, k );
         if ( l.kind != c )
            continue;
         L.type[L.n] = t, L.row[L.n] = k, L.ox[L.n] = l.ox, L.oy[L.n] = l.oy, L.oz[L.n] = l.oz;
         ++L.n;
      }
   return L;
}
template < int C >
struct DkCellsOf
{
   static constexpr DkCellList value = dk_cells( C );
};
template < int T, int D >
struct DkLocalOf
{
   static constexpr CLocal value = c_local( T, D );
};

// a DoF is inner if no face of the macro-cell holds all its end points
template < int C >
__device__ __forceinline__ bool dk_inner( int N, int x, int y, int z )
{
   if constexpr ( C == 0 )
      return x > 0 && y > 0 && z > 0 && x + y + z < N - 1;
   else
   {
      constexpr int ax = kEdgeEndsHost[C - 1][0][0], ay = kEdgeEndsHost[C - 1][0][1], az = kEdgeEndsHost[C - 1][0][2];
      constexpr int bx = kEdgeEndsHost[C - 1][1][0], by = kEdgeEndsHost[C - 1][1][1], bz = kEdgeEndsHost[C - 1][1][2];
      const bool    f0 = z + az == 0 && z + bz == 0, f1 = y + ay == 0 && y + by == 0, f2 = x + ax == 0 && x + bx == 0;
      const bool    f3 = x + y + z + ( ax + ay + az ) == N - 1 && x + y + z + ( bx + by + bz ) == N - 1;
      return !( f0 || f1 || f2 || f3 );
   }
}

// Index arithmetic of the inner form.  Every value a thread reads sits at a compile-time offset ( DX, DY, DZ ) from the thread's own
// logical index ( x, y, z ) in an array of width N ( vertex DoFs ), n ( edge DoFs X .. YZ ) or n - 1 ( XYZ ).  The index of ( x, y, z )
// itself is formed once per width; with Wz = width - z the layout  index = tet( W ) - tet( Wz ) + y Wz - y ( y - 1 ) / 2 + x  gives
//    index( x + DX, y + DY, z + DZ ) - index( x, y, z ) = DX + tet( Wz ) - tet( Wz - DZ ) + DY ( Wz - y ) - DZ y - DY DZ - ( DY^2 - DY ) / 2,
// a polynomial identity (the base index need not be a valid entry).  Per load that is a handful of 32-bit operations, shared where
// ( DY, DZ ) repeat.
struct DkBase
{
   int b[3], wz[3]; // by width: 0: N, 1: n, 2: n - 1
   int y, te;       // te = tet( n ): length of an edge block
};
__device__ __forceinline__ int dk_tet( int w ) { return ( w * ( w + 1 ) * ( w + 2 ) ) / 6; }
__device__ __forceinline__ DkBase dk_base( int N, int x, int y, int z )
{
   DkBase B;
#pragma unroll
   for ( int s = 0; s < 3; ++s )
   {
      const int W = N - s, wz = W - z;
      B.wz[s]     = wz;
      B.b[s]      = dk_tet( W ) - dk_tet( wz ) + y * wz - ( y * ( y - 1 ) ) / 2 + x;
   }
   B.y = y, B.te = dk_tet( N - 1 );
   return B;
}
template < int K, int DX, int DY, int DZ >
__device__ __forceinline__ int dk_at( const DkBase& B )
{
   static_assert( DZ >= -2 && DZ <= 2, "offsets of the DoFs of a micro-cell" );
   constexpr int S  = K == 0 ? 0 : ( K == 7 ? 2 : 1 );
   const int     wz = B.wz[S], y = B.y;
   int           sl = 0;
   if constexpr ( DZ == 1 )
      sl = tri( wz );
   else if constexpr ( DZ == -1 )
      sl = -tri( wz + 1 );
   else if constexpr ( DZ == 2 )
      sl = tri( wz ) + tri( wz - 1 );
   else if constexpr ( DZ == -2 )
      sl = -tri( wz + 1 ) - tri( wz + 2 );
   const int at = B.b[S] + DX + sl + DY * ( wz - y ) - DZ * y - DY * DZ - ( DY * DY - DY ) / 2;
   return K == 0 ? at : ( K - 1 ) * B.te + at;
}

template < int C, int I >
__device__ __forceinline__ void dk_inner_cell( const DkArgs& A, const DkBase& B, double& acc )
{
   constexpr int T = DkCellsOf< C >::value.type[I], ROW = DkCellsOf< C >::value.row[I];
   constexpr int MX = -DkCellsOf< C >::value.ox[I], MY = -DkCellsOf< C >::value.oy[I], MZ = -DkCellsOf< C >::value.oz[I];
   double        k[10], u[10];
   [&]< int... D >( std::integer_sequence< int, D... > ) {
      const int at[10] = { dk_at< DkLocalOf< T, D >::value.kind, MX + DkLocalOf< T, D >::value.ox, MY + DkLocalOf< T, D >::value.oy,
                                  MZ + DkLocalOf< T, D >::value.oz >( B )... };
      ( ( k[D] = ( DkLocalOf< T, D >::value.kind == 0 ? A.kV : A.kE )[at[D]] ), ... );
      ( ( u[D] = ( DkLocalOf< T, D >::value.kind == 0 ? A.srcV : A.srcE )[at[D]] ), ... );
   }
   ( std::make_integer_sequence< int, 10 >{} );
   acc += A.alpha * dk_element_row( A.W.g[T], k, u, ROW );
   // one micro-cell at a time: the 24 cells of a vertex DoF read 480 values, which must not all be in flight at once
   __builtin_amdgcn_sched_barrier( 0 );
}

template < int C >
__device__ __forceinline__ void dk_inner_body( const DkArgs& A )
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
   const DkBase B   = dk_base( N, x, y, z );
   double       acc = 0.0;
   [&]< int... I >( std::integer_sequence< int, I... > ) { ( dk_inner_cell< C, I >( A, B, acc ), ... ); }
   ( std::make_integer_sequence< int, NC >{} );
   double* out = C == 0 ? A.dstV + q : A.dstE + ( C - 1 ) * B.te + q;
   *out        = A.update == HYTEG_HIP_ADD ? *out + acc : acc;
}

// the inner vertex DoFs (24 micro-cells each, the most registers) and, blockIdx.y + 1 = destination kind, the inner edge DoFs of the
// kinds of A.kinds: two launches, so that the edge kinds are not held to the vertex kind's occupancy
__global__ __launch_bounds__( kThreads ) void p2_divkgrad_inner_vertex_kernel( const DkArgs A ) { dk_inner_body< 0 >( A ); }
__global__ __launch_bounds__( kThreads ) void p2_divkgrad_inner_edge_kernel( const DkArgs A )
{
   const int c = blockIdx.y + 1;
   if ( !( ( A.kinds >> c ) & 1u ) )
      return;
   switch ( c )
   {
   case 1:
      dk_inner_body< 1 >( A );
      break;
   case 2:
      dk_inner_body< 2 >( A );
      break;
   case 3:
      dk_inner_body< 3 >( A );
      break;
   case 4:
      dk_inner_body< 4 >( A );
      break;
   case 5:
      dk_inner_body< 5 >( A );
      break;
   case 6:
      dk_inner_body< 6 >( A );
      break;
   default:
      dk_inner_body< 7 >( A );
      break;
   }
}

} // namespace
