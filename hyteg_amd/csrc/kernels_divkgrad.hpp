// Kernels of the variable-coefficient P1 diffusion operator  -div( k grad u )  on one macro-cell (p1_divkgrad.hip).
// Replaces apply_macro_3D and computeInverseDiagonalOperatorValues_macro_3D of the generated
// operatorgeneration::P1ElementwiseDivKGrad (module hyteg_operators; its source is absent from the snapshot, the class is used in
// tests/hyteg/convergence/ElementwiseDivKGradCGConvergenceTest.cpp).  With k linear on a micro-cell e and constant shape-function
// gradients the element matrix is  A_e = mean( k at the 4 vertices of e ) * K_e,  K_e the P1 Laplace element matrix of the
// micro-cell's type (element_matrices.hpp).  K_e has zero row sums, so the value at a point p is
//    sum over the micro-cells e at p:  mean_k( e ) * sum over the three other vertices j of e:  K_e[p, j] * ( u_j - u_p ),
// i.e. 14 differences, one k-sum and three weights per adjacent micro-cell.  The weights depend on ( type, vertex pair ) only:
// 36 wave-uniform doubles in the kernel arguments (with the 1/4 of the mean folded in), never a per-lane table.
//
// Two kernels:
//  * divkgrad_zmarch_kernel: the inner points (24 micro-cells each), a register z-march in the manner of kernels_apply_zmarch.hpp.
//    A wave owns a brick of NY rows x 64 x-positions x LZ slices, loads every row segment of src AND of k once through buffer
//    loads with wave-uniform bases, keeps the live slices of both in registers and stores dst nontemporally.  The x-1 / x+1
//    neighbours are DPP wave shifts of the loaded src and k rows themselves: mean_k * K * u is not linear in a partial sum that
//    could be shifted instead, as the constant-stencil kernel does.
//  * divkgrad_point_kernel: one thread per point, testing which of the point's 24 micro-cells lie inside the macro-cell
//    (the shell classes, levels 0 and 1, the diagonal; over the inner points it is the form the z-march is measured against).
#pragma once

#include "element_matrices.hpp"
#include "kernels_apply_zmarch.hpp"
#include "shell.hpp"

namespace hyteg_hip {
namespace divkgrad {

// 0.25 * K_t[a][b], a < b, pairs in the order (0,1) (0,2) (0,3) (1,2) (1,3) (2,3); the diagonal 0.25 * K_t[a][a] for the point kernel
struct Weights
{
   double off[6][6];
   double diag[6][4];
};

constexpr int pair_index( int a, int b )
{
   const int lo = a < b ? a : b, hi = a < b ? b : a;
   return lo == 0 ? hi - 1 : ( lo == 1 ? hi + 1 : 5 );
}
constexpr int micro_vert( int t, int k, int r )
{
   constexpr int V[6][4][3] = { { { 0, 0, 0 }, { 1, 0, 0 }, { 0, 1, 0 }, { 0, 0, 1 } }, { { 1, 0, 0 }, { 1, 1, 0 }, { 0, 1, 0 }, { 1, 0, 1 } },
                                { { 1, 0, 0 }, { 0, 1, 0 }, { 1, 0, 1 }, { 0, 0, 1 } }, { { 1, 1, 0 }, { 1, 1, 1 }, { 0, 1, 1 }, { 1, 0, 1 } },
                                { { 1, 0, 1 }, { 0, 1, 1 }, { 0, 0, 1 }, { 0, 1, 0 } }, { { 0, 1, 0 }, { 1, 1, 0 }, { 1, 0, 1 }, { 0, 1, 1 } } };
   return V[t][k][r]; // = elmat::kMicroCellVerts, usable in constant expressions on the device
}
// index in the 15 stencil directions (C-ABI weight order) of the edge from local vertex i to local vertex j of a type-t micro-cell
constexpr int edge_dir( int t, int i, int j )
{
   const int dx = micro_vert( t, j, 0 ) - micro_vert( t, i, 0 ), dy = micro_vert( t, j, 1 ) - micro_vert( t, i, 1 ),
             dz = micro_vert( t, j, 2 ) - micro_vert( t, i, 2 );
   for ( int k = 0; k < 15; ++k )
      if ( kStencilOffsC[k][0] == dx && kStencilOffsC[k][1] == dy && kStencilOffsC[k][2] == dz )
         return k;
   return -1;
}

// the sum over the 24 micro-cells at an inner point.  d[15]: the differences u_j - u_p to the point's stencil neighbours, k[15]: the
// coefficient there (index 7: the point itself).  Cell C = 4 t + i is the type-t micro-cell that has the point as its local vertex i.
template < int C >
__device__ inline double cell_term( const Weights& W, const double ( &d )[15], const double ( &k )[15] )
{
   constexpr int t = C / 4, i = C % 4;
   constexpr int ja = ( i + 1 ) % 4, jb = ( i + 2 ) % 4, jc = ( i + 3 ) % 4;
   constexpr int a = edge_dir( t, i, ja ), b = edge_dir( t, i, jb ), c = edge_dir( t, i, jc );
   static_assert( a >= 0 && b >= 0 && c >= 0 && a != 7 && b != 7 && c != 7, "every micro-cell edge is a stencil direction" );
   const double m = ( k[7] + k[a] ) + ( k[b] + k[c] );
   double       g = W.off[t][pair_index( i, ja )] * d[a];
   g              = fma( W.off[t][pair_index( i, jb )], d[b], g );
   g              = fma( W.off[t][pair_index( i, jc )], d[c], g );
   return m * g;
}
template < int... Cs >
__device__ inline double inner_sum( const Weights& W, const double ( &d )[15], const double ( &k )[15], std::integer_sequence< int, Cs... > )
{
   double acc = 0.0;
   ( ( acc += cell_term< Cs >( W, d, k ) ), ... );
   return acc;
}

enum Mode
{
   DKG_REPLACE = 0,
   DKG_ADD     = 1,
   DKG_JACOBI  = 2, // dst = src + omega * invdiag * ( rhs - A src )
   DKG_DIAG    = 3  // dst += diagonal (point kernel only; src unused)
};

struct Args
{
   double*       dst;
   const double* src;
   const double* k;
   const double* rhs;     // JACOBI
   const double* invdiag; // JACOBI
   unsigned      bytes;   // size of a cell array in bytes (buffer range)
   int           N;       // 2^level + 1
   double        omega;
   Weights       W;
};

template < int MODE, int NY, int LZ, int PFD >
__global__ __launch_bounds__( 64 * kZMarchWavesPerBlock ) void divkgrad_zmarch_kernel( const BrickTask* tasks, int ntasks, int xcd_chunk, const Args A )
{
   static_assert( LZ + 2 <= kBrickMaxSlices, "the table carries the slice bases of bricks of up to kBrickMaxSlices - 2 slices" );
   int b = blockIdx.x;
   if ( xcd_chunk > 0 )
      b = ( blockIdx.x & 7 ) * xcd_chunk + ( blockIdx.x >> 3 );
   const int task = __builtin_amdgcn_readfirstlane( b * kZMarchWavesPerBlock + ( threadIdx.x >> 6 ) );
   if ( task >= ntasks )
      return;
   const BrickTask t    = tasks[task];
   const int       lane = threadIdx.x & 63;

   constexpr int                kStAux = 2; // nontemporal
   const __amdgpu_buffer_rsrc_t rs     = __builtin_amdgcn_make_buffer_rsrc( const_cast< double* >( A.src ), 0, A.bytes, 0x00020000 );
   const __amdgpu_buffer_rsrc_t rk     = __builtin_amdgcn_make_buffer_rsrc( const_cast< double* >( A.k ), 0, A.bytes, 0x00020000 );
   const __amdgpu_buffer_rsrc_t rd     = __builtin_amdgcn_make_buffer_rsrc( A.dst, 0, A.bytes, 0x00020000 );
   const __amdgpu_buffer_rsrc_t rr = __builtin_amdgcn_make_buffer_rsrc( const_cast< double* >( MODE == DKG_JACOBI ? A.rhs : A.src ), 0, A.bytes, 0x00020000 );
   const __amdgpu_buffer_rsrc_t ri =
       __builtin_amdgcn_make_buffer_rsrc( const_cast< double* >( MODE == DKG_JACOBI ? A.invdiag : A.src ), 0, A.bytes, 0x00020000 );

   const int lane_off = lane * 8;
   const int ym       = t.y0 - 1;

   // U / K[q][r]: src / k at slice z0-1+q, row ym+r, x = xb + lane.  Lanes beyond the end of a row re-read its last entry; a row
   // that does not exist has a negative bound and is dropped by the range check (as in zmarch_body).
   double U[LZ + 2][NY + 2], K[LZ + 2][NY + 2];
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
            U[q][r]         = zm_load2< double >( rs, vo, ix * 8 );
            K[q][r]         = zm_load2< double >( rk, vo, ix * 8 );
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

   // the second and third array of Add / Jacobi at the output points, PFD slices ahead of their use like the source slices
   double EX0[LZ][NY], EX1[LZ][NY];
   auto   load_extra = [&]( auto sc ) {
      constexpr int s = decltype( sc )::value;
      constexpr int q = s + 1;
      if constexpr ( MODE != DKG_REPLACE )
      {
         const int W  = Wqs[q];
         int       ie = baseq[q] + ( W - ym ); // (xb, y0, z)
#pragma unroll
         for ( int j = 0; j < NY; ++j )
         {
            const int last8 = ( W - ( t.y0 + j ) - 1 - t.xb ) * 8;
            const int vo    = min( lane_off, last8 );
            if constexpr ( MODE == DKG_ADD )
               EX0[s][j] = zm_load2< double, 2 >( rd, vo, ie * 8 ); // read once, rewritten right after: nontemporal
            else
            {
               EX0[s][j] = zm_load2< double >( rr, vo, ie * 8 );
               EX1[s][j] = zm_load2< double >( ri, vo, ie * 8 );
            }
            ie += W - ( t.y0 + j );
         }
      }
   };
   if constexpr ( MODE != DKG_REPLACE )
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
         // the 15 stencil values of src and k in the C-ABI's direction order; rows: j = y - 1, j + 1 = y, j + 2 = y + 1
         double u[15], k[15];
#define HH_DKG_GATHER( v, S )                     \
   v[0]  = S[q - 1][j + 1];                       \
   v[1]  = zm_lane_plus_1( S[q - 1][j + 1] );     \
   v[2]  = zm_lane_minus_1( S[q - 1][j + 2] );    \
   v[3]  = S[q - 1][j + 2];                       \
   v[4]  = S[q][j];                               \
   v[5]  = zm_lane_plus_1( S[q][j] );             \
   v[6]  = zm_lane_minus_1( S[q][j + 1] );        \
   v[7]  = S[q][j + 1];                           \
   v[8]  = zm_lane_plus_1( S[q][j + 1] );         \
   v[9]  = zm_lane_minus_1( S[q][j + 2] );        \
   v[10] = S[q][j + 2];                           \
   v[11] = S[q + 1][j];                           \
   v[12] = zm_lane_plus_1( S[q + 1][j] );         \
   v[13] = zm_lane_minus_1( S[q + 1][j + 1] );    \
   v[14] = S[q + 1][j + 1];
         HH_DKG_GATHER( u, U )
         HH_DKG_GATHER( k, K )
#undef HH_DKG_GATHER
         const double a0 = u[7];
#pragma unroll
         for ( int n = 0; n < 15; ++n )
            u[n] = u[n] - a0; // the differences u_j - u_p
         const double acc = inner_sum( A.W, u, k, std::make_integer_sequence< int, 24 >{} );

         const int R = W - ( t.y0 + j );
         double    out;
         if constexpr ( MODE == DKG_REPLACE )
            out = acc;
         else if constexpr ( MODE == DKG_ADD )
            out = acc + EX0[s][j];
         else
            out = a0 + A.omega * ( EX1[s][j] * ( EX0[s][j] - acc ) );
         // outputs are lanes 1 .. min( 62, R - 2 - xb ) of slices that exist
         const int      cnt = s < t.nz ? min( 62, R - 2 - t.xb ) : 0; // wave-uniform
         const unsigned lm1 = (unsigned) ( lane - 1 );
         const bool     on  = lm1 < (unsigned) max( cnt, 0 );
         zm_store2< double, kStAux >( rd, on ? lane_off : -8, io * 8, out );
         io += R;
      }
   };
   [&]< int... Is >( std::integer_sequence< int, Is... > ) { ( step( std::integral_constant< int, Is >{} ), ... ); }
   ( std::make_integer_sequence< int, LZ >{} );
}

// this cell's share at point (x, y, z): the sum over those of the 24 micro-cells at the point that lie inside the macro-cell.
// Returns the apply ( DIAG == false ) or the diagonal entry ( DIAG == true ).
template < bool DIAG >
__device__ inline double point_share( const Weights& W, const double* __restrict__ src, const double* __restrict__ kk, int N, int x, int y, int z )
{
   const int    i0 = cell_index( N, x, y, z );
   const int    w  = N - z;
   const double kp = kk[i0];
   const double up = DIAG ? 0.0 : src[i0];
   double       acc = 0.0;
#pragma unroll
   for ( int t = 0; t < 6; ++t )
#pragma unroll
      for ( int i = 0; i < 4; ++i )
      {
         // the type-t micro-cell with the point as local vertex i: all four vertices inside the macro-cell?
         bool   inside = true;
         int    idx[4];
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
         double m = kp, g = 0.0;
#pragma unroll
         for ( int j = 0; j < 4; ++j )
            if ( j != i )
            {
               m += kk[idx[j]];
               if ( !DIAG )
                  g = fma( W.off[t][pair_index( i, j )], src[idx[j]] - up, g );
            }
         acc += DIAG ? m * W.diag[t][i] : m * g;
      }
   return acc;
}

constexpr int kPointThreads = 256;

// the shell classes of `mask` (enumeration of shell.hpp)
template < int MODE >
__global__ __launch_bounds__( kPointThreads ) void divkgrad_shell_kernel( const Args A, unsigned mask )
{
   const int q = blockIdx.x * kPointThreads + threadIdx.x;
   int       x, y, z, slot;
   if ( !shell::shell_point( A.N, q, x, y, z, slot ) || !( ( mask >> slot ) & 1u ) )
      return;
   const double acc = point_share< MODE == DKG_DIAG >( A.W, A.src, A.k, A.N, x, y, z );
   const int    i   = cell_index( A.N, x, y, z );
   A.dst[i]         = MODE == DKG_REPLACE ? acc : acc + A.dst[i];
}

// the inner points, one thread per point over the inner tiles (the diagonal; the comparison form of the z-march)
template < int MODE >
__global__ __launch_bounds__( kPointThreads ) void divkgrad_inner_point_kernel( const Args A, const Tile* tiles, int ntiles )
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
      const double acc = point_share< MODE == DKG_DIAG >( A.W, A.src, A.k, N, x, y, tl.z );
      double       out;
      if ( MODE == DKG_REPLACE )
         out = acc;
      else if ( MODE == DKG_JACOBI )
         out = A.src[i] + A.omega * ( A.invdiag[i] * ( A.rhs[i] - acc ) );
      else
         out = acc + A.dst[i];
      A.dst[i] = out;
   }
}

} // namespace divkgrad
} // namespace hyteg_hip
