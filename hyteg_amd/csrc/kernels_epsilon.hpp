// Kernels of the variable-viscosity P1 epsilon operator  -div( 2 mu eps(u) ),  eps(u) = ( grad u + grad u^T ) / 2,  on one macro-cell
// (p1_epsilon.hip).  Replaces the nine P1ElementwiseOperator blocks of P1ElementwiseAffineEpsilonOperator
// (src/mixed_operator/P1EpsilonOperator.hpp:89-164) by one pass over u, v, w and mu.
// With mu linear on a micro-cell e and constant barycentric gradients g_a the block for test component i, trial component j is
//    A_e^{ij}[a][b] = mean( mu at the 4 vertices of e ) * |e| * ( delta_ij g_a . g_b + g_a[j] g_b[i] ).
// Every block has zero row sums ( sum_b g_b = 0 ), so the value at a point p = local vertex a of e needs only the differences
// d^j_b = u^j_b - u^j_p.  Two wave-uniform weight forms (template parameter FORM of the z-march):
//  * FORM 0, gradients: h_a = sqrt( |e| / 4 ) g_a, 6 x 4 x 3 doubles in the kernel arguments.  Per micro-cell
//       D[j][r] = sum_b h_b[r] d^j_b   ( = sqrt( |e| / 4 ) d_r u^j ),   out_i += musum * sum_r h_a[r] ( D[i][r] + D[r][i] );
//  * FORM 1, blocks: the 6 x 4 x 3 x 3 x 3 products  |e| / 4 ( delta_ij g_a . g_b + g_a[j] g_b[i] )  in a device table read through
//    scalar loads,  out_i += musum * sum_j sum_b T[t][a][i][j][b] d^j_b.
// Kernels, as in kernels_divkgrad.hpp: epsilon_zmarch_kernel (inner points: a register z-march that loads every row segment of u, v,
// w and mu once, takes x -+ 1 by DPP shifts, forms each adjacent micro-cell's mu-sum once for the three destination components and
// stores them nontemporally) and the one-thread-per-point kernels (shell classes, levels 0-1, the three diagonals, and the inner
// points as the second implementation the z-march is compared against).
#pragma once

#include "kernels_divkgrad.hpp"

namespace hyteg_hip {
namespace epsilon {

using divkgrad::edge_dir;
using divkgrad::micro_vert;

// h[t][a][r] = sqrt( |e_t| / 4 ) * d_r ( barycentric function a of the type-t micro-cell )
struct Weights
{
   double h[6][4][3];
};
constexpr int kTableDoubles = 6 * 4 * 3 * 3 * 3; // FORM 1: T[t][a][i][j][n], n: the vertices ( a + 1 + n ) % 4

enum Mode
{
   EPS_REPLACE = 0,
   EPS_ADD     = 1,
   EPS_JACOBI  = 2, // dst_i = src_i + omega * invdiag_i * ( rhs_i - ( A src )_i )
   EPS_DIAG    = 3  // dst_i += diagonal of A^{ii} (point kernels only; src unused)
};

struct Args
{
   double*       dst[3];
   const double* src[3];
   const double* mu;
   const double* rhs[3];     // JACOBI
   const double* invdiag[3]; // JACOBI
   const double* table;      // FORM 1
   unsigned      bytes;      // size of a cell array in bytes (buffer range)
   int           N;          // 2^level + 1
   unsigned      comps;      // z-march / inner point kernel: bit i = destination component i is written
   unsigned      masks[3];   // shell kernel: the class mask of each destination component
   double        omega;
   Weights       W;
};

typedef const double __attribute__( ( address_space( 4 ) ) ) table_double_t;

// one adjacent micro-cell of an inner point.  d[j][15]: the differences of component j to the stencil neighbours, k[15]: mu there.
// Cell C = 4 t + i is the type-t micro-cell that has the point as its local vertex i.
template < int FORM, int C >
__device__ inline void cell_term( const Args& A, const double ( &d )[3][15], const double ( &k )[15], double ( &acc )[3] )
{
   constexpr int t = C / 4, i = C % 4;
   constexpr int ja = ( i + 1 ) % 4, jb = ( i + 2 ) % 4, jc = ( i + 3 ) % 4;
   constexpr int a = edge_dir( t, i, ja ), b = edge_dir( t, i, jb ), c = edge_dir( t, i, jc );
   static_assert( a >= 0 && b >= 0 && c >= 0 && a != 7 && b != 7 && c != 7, "every micro-cell edge is a stencil direction" );
   const double m = ( k[7] + k[a] ) + ( k[b] + k[c] );
   if constexpr ( FORM == 0 )
   {
      const double( &h )[4][3] = A.W.h[t];
      double D[3][3];
#pragma unroll
      for ( int j = 0; j < 3; ++j )
#pragma unroll
         for ( int r = 0; r < 3; ++r )
            D[j][r] = fma( h[jc][r], d[j][c], fma( h[jb][r], d[j][b], h[ja][r] * d[j][a] ) );
#pragma unroll
      for ( int ic = 0; ic < 3; ++ic )
      {
         double s = h[i][0] * ( D[ic][0] + D[0][ic] );
         s        = fma( h[i][1], D[ic][1] + D[1][ic], s );
         s        = fma( h[i][2], D[ic][2] + D[2][ic], s );
         acc[ic]  = fma( m, s, acc[ic] );
      }
   }
   else
   {
      table_double_t* T = (table_double_t*) A.table + C * 27;
#pragma unroll
      for ( int ic = 0; ic < 3; ++ic )
      {
         double s = 0.0;
#pragma unroll
         for ( int j = 0; j < 3; ++j )
         {
            s = fma( T[( ic * 3 + j ) * 3 + 0], d[j][a], s );
            s = fma( T[( ic * 3 + j ) * 3 + 1], d[j][b], s );
            s = fma( T[( ic * 3 + j ) * 3 + 2], d[j][c], s );
         }
         acc[ic] = fma( m, s, acc[ic] );
      }
   }
}
template < int FORM, int... Cs >
__device__ inline void inner_sum( const Args& A, const double ( &d )[3][15], const double ( &k )[15], double ( &acc )[3], std::integer_sequence< int, Cs... > )
{
   ( cell_term< FORM, Cs >( A, d, k, acc ), ... );
}

template < int MODE, int NY, int LZ, int FORM >
__global__ __launch_bounds__( 64 * kZMarchWavesPerBlock ) void epsilon_zmarch_kernel( const BrickTask* tasks, int ntasks, int xcd_chunk, const Args A )
{
   static_assert( LZ + 2 <= kBrickMaxSlices, "the table carries the slice bases of bricks of up to kBrickMaxSlices - 2 slices" );
   constexpr int PFD = 1; // loads run one slice ahead
   int           b   = blockIdx.x;
   if ( xcd_chunk > 0 )
      b = ( blockIdx.x & 7 ) * xcd_chunk + ( blockIdx.x >> 3 );
   const int task = __builtin_amdgcn_readfirstlane( b * kZMarchWavesPerBlock + ( threadIdx.x >> 6 ) );
   if ( task >= ntasks )
      return;
   const BrickTask t    = tasks[task];
   const int       lane = threadIdx.x & 63;

   constexpr int          kStAux = 2; // nontemporal
   __amdgpu_buffer_rsrc_t rs[4], rd[3], rr[3], ri[3]; // sources (3: mu), destinations, rhs, inverse diagonals
#pragma unroll
   for ( int c = 0; c < 3; ++c )
   {
      rs[c] = __builtin_amdgcn_make_buffer_rsrc( const_cast< double* >( A.src[c] ), 0, A.bytes, 0x00020000 );
      rd[c] = __builtin_amdgcn_make_buffer_rsrc( A.dst[c], 0, A.bytes, 0x00020000 );
      rr[c] = __builtin_amdgcn_make_buffer_rsrc( const_cast< double* >( MODE == EPS_JACOBI ? A.rhs[c] : A.src[c] ), 0, A.bytes, 0x00020000 );
      ri[c] = __builtin_amdgcn_make_buffer_rsrc( const_cast< double* >( MODE == EPS_JACOBI ? A.invdiag[c] : A.src[c] ), 0, A.bytes, 0x00020000 );
   }
   rs[3] = __builtin_amdgcn_make_buffer_rsrc( const_cast< double* >( A.mu ), 0, A.bytes, 0x00020000 );

   const int lane_off = lane * 8;
   const int ym       = t.y0 - 1;

   // S[c][q][r]: u, v, w, mu ( c = 0..3 ) at slice z0-1+q, row ym+r, x = xb + lane.  Lanes beyond the end of a row re-read its last
   // entry; a row that does not exist has a negative bound and is dropped by the range check (as in divkgrad_zmarch_kernel).
   double S[4][LZ + 2][NY + 2];
   auto   load_slice = [&]( auto qc, int base_q, int W_q ) {
      constexpr int q  = decltype( qc )::value;
      int           ix = base_q;
#pragma unroll
      for ( int r = 0; r < NY + 2; ++r )
      {
         const bool need = ( q == 0 ) ? ( r >= 1 ) : ( q == LZ + 1 ? ( r <= NY ) : true );
         if ( need )
         {
            const int last8 = ( W_q - ( ym + r ) - 1 - t.xb ) * 8;
            const int vo    = min( lane_off, last8 );
#pragma unroll
            for ( int c = 0; c < 4; ++c )
               S[c][q][r] = zm_load2< double >( rs[c], vo, ix * 8 );
         }
         ix += W_q - ( ym + r );
      }
   };
   int baseq[LZ + 2], Wqs[LZ + 2];
#pragma unroll
   for ( int q = 0; q < LZ + 2; ++q )
   {
      baseq[q] = t.base[q];
      Wqs[q]   = t.W0 - q;
   }
   [&]< int... Is >( std::integer_sequence< int, Is... > ) { ( load_slice( std::integral_constant< int, Is >{}, baseq[Is], Wqs[Is] ), ... ); }
   ( std::make_integer_sequence < int, ( 2 + PFD <= LZ + 2 ? 2 + PFD : LZ + 2 ) > {} );

   // the further arrays of Add / Jacobi at the output points, PFD slices ahead of their use like the source slices
   double EX0[3][LZ][NY], EX1[3][LZ][NY];
   auto   load_extra = [&]( auto sc ) {
      constexpr int s = decltype( sc )::value;
      constexpr int q = s + 1;
      if constexpr ( MODE != EPS_REPLACE )
      {
         const int W  = Wqs[q];
         int       ie = baseq[q] + ( W - ym ); // (xb, y0, z)
#pragma unroll
         for ( int j = 0; j < NY; ++j )
         {
            const int last8 = ( W - ( t.y0 + j ) - 1 - t.xb ) * 8;
            const int vo    = min( lane_off, last8 );
#pragma unroll
            for ( int c = 0; c < 3; ++c )
            {
               if constexpr ( MODE == EPS_ADD )
                  EX0[c][s][j] = zm_load2< double, 2 >( rd[c], vo, ie * 8 ); // read once, rewritten right after: nontemporal
               else
               {
                  EX0[c][s][j] = zm_load2< double >( rr[c], vo, ie * 8 );
                  EX1[c][s][j] = zm_load2< double >( ri[c], vo, ie * 8 );
               }
            }
            ie += W - ( t.y0 + j );
         }
      }
   };
   if constexpr ( MODE != EPS_REPLACE )
   {
      [&]< int... Is >( std::integer_sequence< int, Is... > ) { ( load_extra( std::integral_constant< int, Is >{} ), ... ); }
      ( std::make_integer_sequence < int, ( PFD < LZ ? PFD : LZ ) > {} );
   }

   auto step = [&]( auto sc ) {
      constexpr int s = decltype( sc )::value; // output slice z0 + s, centre q = s + 1
      constexpr int q = s + 1;
      if constexpr ( q + 1 + PFD <= LZ + 1 )
         load_slice( std::integral_constant< int, q + 1 + PFD >{}, baseq[q + 1 + PFD], Wqs[q + 1 + PFD] );
      if constexpr ( s + PFD < LZ )
         load_extra( std::integral_constant< int, s + PFD >{} );

      const int W  = Wqs[q];
      int       io = baseq[q] + ( W - ym ); // (xb, y0, z)
#pragma unroll
      for ( int j = 0; j < NY; ++j )
      {
         // the 15 stencil values of u, v, w and mu in the C-ABI's direction order; rows: j = y - 1, j + 1 = y, j + 2 = y + 1
         double u[3][15], k[15];
#define HH_EPS_GATHER( v, P )                     \
   v[0]  = P[q - 1][j + 1];                       \
   v[1]  = zm_lane_plus_1( P[q - 1][j + 1] );     \
   v[2]  = zm_lane_minus_1( P[q - 1][j + 2] );    \
   v[3]  = P[q - 1][j + 2];                       \
   v[4]  = P[q][j];                               \
   v[5]  = zm_lane_plus_1( P[q][j] );             \
   v[6]  = zm_lane_minus_1( P[q][j + 1] );        \
   v[7]  = P[q][j + 1];                           \
   v[8]  = zm_lane_plus_1( P[q][j + 1] );         \
   v[9]  = zm_lane_minus_1( P[q][j + 2] );        \
   v[10] = P[q][j + 2];                           \
   v[11] = P[q + 1][j];                           \
   v[12] = zm_lane_plus_1( P[q + 1][j] );         \
   v[13] = zm_lane_minus_1( P[q + 1][j + 1] );    \
   v[14] = P[q + 1][j + 1];
         HH_EPS_GATHER( u[0], S[0] )
         HH_EPS_GATHER( u[1], S[1] )
         HH_EPS_GATHER( u[2], S[2] )
         HH_EPS_GATHER( k, S[3] )
#undef HH_EPS_GATHER
         double a0[3];
#pragma unroll
         for ( int c = 0; c < 3; ++c )
         {
            a0[c] = u[c][7];
#pragma unroll
            for ( int n = 0; n < 15; ++n )
               u[c][n] = u[c][n] - a0[c]; // the differences u_j - u_p
         }
         double acc[3] = { 0.0, 0.0, 0.0 };
         inner_sum< FORM >( A, u, k, acc, std::make_integer_sequence< int, 24 >{} );

         const int R = W - ( t.y0 + j );
         // outputs are lanes 1 .. min( 62, R - 2 - xb ) of slices that exist
         const int      cnt = s < t.nz ? min( 62, R - 2 - t.xb ) : 0; // wave-uniform
         const unsigned lm1 = (unsigned) ( lane - 1 );
         const bool     on  = lm1 < (unsigned) max( cnt, 0 );
#pragma unroll
         for ( int c = 0; c < 3; ++c )
         {
            double out;
            if constexpr ( MODE == EPS_REPLACE )
               out = acc[c];
            else if constexpr ( MODE == EPS_ADD )
               out = acc[c] + EX0[c][s][j];
            else
               out = a0[c] + A.omega * ( EX1[c][s][j] * ( EX0[c][s][j] - acc[c] ) );
            const bool write = on && ( ( A.comps >> c ) & 1u );
            zm_store2< double, kStAux >( rd[c], write ? lane_off : -8, io * 8, out );
         }
         io += R;
      }
   };
   [&]< int... Is >( std::integer_sequence< int, Is... > ) { ( step( std::integral_constant< int, Is >{} ), ... ); }
   ( std::make_integer_sequence< int, LZ >{} );
}

// this cell's share at point (x, y, z): the sum over those of the 24 micro-cells at the point that lie inside the macro-cell, in the
// gradient form.  acc: the three components of the apply ( DIAG == false ) or the diagonal entries of A^{ii} ( DIAG == true ).
template < bool DIAG >
__device__ inline void point_share( const Args& A, int x, int y, int z, double ( &acc )[3] )
{
   const int     N  = A.N;
   const int     i0 = cell_index( N, x, y, z );
   const int     w  = N - z;
   const double* kk = A.mu;
   const double  kp = kk[i0];
   double        up[3];
#pragma unroll
   for ( int c = 0; c < 3; ++c )
   {
      up[c]  = DIAG ? 0.0 : A.src[c][i0];
      acc[c] = 0.0;
   }
#pragma unroll
   for ( int t = 0; t < 6; ++t )
#pragma unroll
      for ( int i = 0; i < 4; ++i )
      {
         // the type-t micro-cell with the point as local vertex i: all four vertices inside the macro-cell?
         bool inside = true;
         int  idx[4];
#pragma unroll
         for ( int j = 0; j < 4; ++j )
         {
            const int dx = micro_vert( t, j, 0 ) - micro_vert( t, i, 0 ), dy = micro_vert( t, j, 1 ) - micro_vert( t, i, 1 ),
                      dz = micro_vert( t, j, 2 ) - micro_vert( t, i, 2 );
            const int nx = x + dx, ny = y + dy, nz = z + dz;
            inside       = inside && nx >= 0 && ny >= 0 && nz >= 0 && nx + ny + nz <= N - 1;
            // layout algebra of shell::share
            const int rowDelta   = dy == 0 ? 0 : ( dy > 0 ? ( w - y ) : -( w - y + 1 ) );
            const int sliceDelta = dz == 0 ? 0 : ( dz > 0 ? tri( w ) - ny : ny - tri( w + 1 ) );
            idx[j]               = i0 + sliceDelta + rowDelta + dx;
         }
         if ( !inside )
            continue;
         const double( &h )[4][3] = A.W.h[t];
         double m = kp, D[3][3] = {};
#pragma unroll
         for ( int j = 0; j < 4; ++j )
            if ( j != i )
            {
               m += kk[idx[j]];
               if ( !DIAG )
#pragma unroll
                  for ( int c = 0; c < 3; ++c )
                  {
                     const double dd = A.src[c][idx[j]] - up[c];
#pragma unroll
                     for ( int r = 0; r < 3; ++r )
                        D[c][r] = fma( h[j][r], dd, D[c][r] );
                  }
            }
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
}

constexpr int kPointThreads = 256;

// the shell classes of A.masks (enumeration of shell.hpp); a component is written where its own mask selects the point's class
template < int MODE >
__global__ __launch_bounds__( kPointThreads ) void epsilon_shell_kernel( const Args A )
{
   const int q = blockIdx.x * kPointThreads + threadIdx.x;
   int       x, y, z, slot;
   if ( !shell::shell_point( A.N, q, x, y, z, slot ) || !( ( ( A.masks[0] | A.masks[1] | A.masks[2] ) >> slot ) & 1u ) )
      return;
   double acc[3];
   point_share< MODE == EPS_DIAG >( A, x, y, z, acc );
   const int i = cell_index( A.N, x, y, z );
#pragma unroll
   for ( int c = 0; c < 3; ++c )
      if ( ( A.masks[c] >> slot ) & 1u )
         A.dst[c][i] = MODE == EPS_REPLACE ? acc[c] : acc[c] + A.dst[c][i];
}

// the inner points, one thread per point over the inner tiles (the diagonals; the comparison form of the z-march)
template < int MODE >
__global__ __launch_bounds__( kPointThreads ) void epsilon_inner_point_kernel( const Args A, const Tile* tiles, int ntiles )
{
   const int tt = blockIdx.x;
   if ( tt >= ntiles )
      return;
   const Tile tl = tiles[tt];
   const int  N = A.N, W = N - tl.z, s0 = slice_start( N, tl.z );
   for ( int e = threadIdx.x; e < tl.cnt; e += kPointThreads )
   {
      const int i = tl.a + e, j = i - s0;
      const int y = row_of( W, j ), x = j - row_start( W, y );
      if ( x < 1 || y < 1 || tl.z < 1 || x + y + tl.z > N - 2 )
         continue;
      double acc[3];
      point_share< MODE == EPS_DIAG >( A, x, y, tl.z, acc );
#pragma unroll
      for ( int c = 0; c < 3; ++c )
      {
         if ( !( ( A.comps >> c ) & 1u ) )
            continue;
         double out;
         if ( MODE == EPS_REPLACE )
            out = acc[c];
         else if ( MODE == EPS_JACOBI )
            out = A.src[c][i] + A.omega * ( A.invdiag[c][i] * ( A.rhs[c][i] - acc[c] ) );
         else
            out = acc[c] + A.dst[c][i];
         A.dst[c][i] = out;
      }
   }
}

} // namespace epsilon
} // namespace hyteg_hip
