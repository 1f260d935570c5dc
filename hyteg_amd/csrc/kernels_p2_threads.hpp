// Thread-per-DoF kernels of the P2 apply with compile-time constant stencils (round 1): p2_inner_kernel for the inner DoFs,
// p2_boundary_kernel for the DoFs on the macro-cell boundary (per-class weight rows), each for one macro-cell and for a batch.
// They are the live path at level 2, the boundary part of kind-restricted applies below level 6, and what
// HYTEG_HIP_P2_INNER_THREADS=1 selects.  Reference: the macro-cell kernels of P2ConstantOperator (vertex-to-vertex, edge-to-vertex,
// vertex-to-edge, edge-to-edge stencils).
#pragma once

#include "p2_common.hpp"

namespace {

// Row bases: every stencil entry of destination kind C reads source kind K at (x + dx, y + dy, z + dz) with compile-time
// (K, dx, dy, dz); the array index of (x, y + dy, z + dz) in kind K's block is computed once per USED (K, dy, dz) and the
// entries add dx.  32-bit index arithmetic: the largest index at level 9 is 6 tet(512) + tet(511) < 2^31.
template < int C >
constexpr bool row_used( int K, int dy, int dz )
{
   constexpr KindStencil S = KindStencilOf< C >::value;
   for ( int q = 0; q < S.n; ++q )
      if ( S.kind[q] == K && S.dy[q] == dy && S.dz[q] == dz )
         return true;
   return false;
}
struct RowBases
{
   int b[8][3][3]; // [source kind][dy + 1][dz + 1]
};
// index of (x, y + DY, z + DZ) from the index i0 of (x, y, z) in a tetrahedral array whose slice z has first-row length Wz:
// (x,y,z) -> (x,y+1,z): + (Wz - y);  (x,y,z) -> (x,y,z+1): + tri(Wz) - y  (the layout algebra of the P1 kernels)
template < int DY, int DZ >
__device__ inline int p2_neighbour_row( int i0, int Wz, int y )
{
   int i = i0, w = Wz;
   if constexpr ( DZ == 1 )
   {
      i += tri( w ) - y;
      w -= 1;
   }
   else if constexpr ( DZ == -1 )
   {
      i -= tri( w + 1 ) - y;
      w += 1;
   }
   if constexpr ( DY == 1 )
      i += w - y;
   else if constexpr ( DY == -1 )
      i -= w - y + 1;
   return i;
}
template < int C, int K, int DY, int DZ >
__device__ inline void p2_row_base( RowBases& R, int i0, int Wz, int y )
{
   if constexpr ( row_used< C >( K, DY, DZ ) )
      R.b[K][DY + 1][DZ + 1] = p2_neighbour_row< DY, DZ >( i0, Wz, y );
}
template < int C, int K >
constexpr bool kind_used()
{
   for ( int dy = -1; dy <= 1; ++dy )
      for ( int dz = -1; dz <= 1; ++dz )
         if ( row_used< C >( K, dy, dz ) )
            return true;
   return false;
}
template < int C, int K >
__device__ inline void p2_row_bases_of_kind( RowBases& R, int N, int n, int x, int y, int z )
{
   if constexpr ( kind_used< C, K >() )
   {
      const int W  = K == 0 ? N : ( K == 7 ? n - 1 : n );
      const int i0 = ( K == 0 ? 0 : ( K - 1 ) * (int) tet32( (unsigned) n ) ) + cell_index( W, x, y, z );
      const int Wz = W - z;
      p2_row_base< C, K, -1, -1 >( R, i0, Wz, y );
      p2_row_base< C, K, 0, -1 >( R, i0, Wz, y );
      p2_row_base< C, K, 1, -1 >( R, i0, Wz, y );
      p2_row_base< C, K, -1, 0 >( R, i0, Wz, y );
      p2_row_base< C, K, 0, 0 >( R, i0, Wz, y );
      p2_row_base< C, K, 1, 0 >( R, i0, Wz, y );
      p2_row_base< C, K, -1, 1 >( R, i0, Wz, y );
      p2_row_base< C, K, 0, 1 >( R, i0, Wz, y );
      p2_row_base< C, K, 1, 1 >( R, i0, Wz, y );
   }
}

template < int C, int Q >
__device__ inline void p2_term( const P2FastArgs& A, const double* __restrict__ w, const RowBases& R, double& acc )
{
   constexpr int K = KindStencilOf< C >::value.kind[Q], DX = KindStencilOf< C >::value.dx[Q], DY = KindStencilOf< C >::value.dy[Q],
                 DZ = KindStencilOf< C >::value.dz[Q];
   static_assert( DY >= -1 && DY <= 1 && DZ >= -1 && DZ <= 1, "stencil offsets" );
   const int idx = R.b[K][DY + 1][DZ + 1] + DX;
   acc           = fma( w[Q], K == 0 ? A.srcV[idx] : A.srcE[idx], acc );
}

// inner DoFs of kind C: inner vertex DoFs x,y,z >= 1, x+y+z <= N-2; inner edge DoFs by EdgeDoFIndexing.hpp:987-1020
template < int C >
__device__ inline bool p2_inner( int N, int x, int y, int z )
{
   const int n = N - 1, s = x + y + z;
   if constexpr ( C == 0 )
      return x >= 1 && y >= 1 && z >= 1 && s <= N - 2;
   else if constexpr ( C == 1 )
      return y > 0 && z > 0 && s < n;
   else if constexpr ( C == 2 )
      return x > 0 && z > 0 && s < n;
   else if constexpr ( C == 3 )
      return x > 0 && y > 0 && s < n;
   else if constexpr ( C == 4 )
      return z > 0 && s < n - 1;
   else if constexpr ( C == 5 )
      return y > 0 && s < n - 1;
   else if constexpr ( C == 6 )
      return x > 0 && s < n - 1;
   else
      return s < n - 1;
}

template < int C >
__device__ inline void p2_inner_body( const P2FastArgs& A )
{
   constexpr int NQ  = KindStencilOf< C >::value.n; // forced constant evaluation: none of the table code may run on the device
   constexpr int OFF = stencil_offset( C );
   const int     N = A.N, n = N - 1;
   const int     W = C == 0 ? N : ( C == 7 ? n - 1 : n );
   const int64_t         i = (int64_t) blockIdx.x * kThreads + threadIdx.x;
   if ( W <= 0 || i >= tet64( W ) )
      return;
   const int z = slice_of( W, i );
   const int j = (int) ( i - ( tet64( W ) - tet64( W - z ) ) );
   const int y = row_of( W - z, j );
   const int x = j - row_start( W - z, y );
   if ( !p2_inner< C >( N, x, y, z ) )
      return;
   const double* __restrict__ w = A.table + OFF;
   double acc                   = 0.0;
   RowBases R;
   [&]< int... K >( std::integer_sequence< int, K... > ) { ( p2_row_bases_of_kind< C, K >( R, N, n, x, y, z ), ... ); }
   ( std::make_integer_sequence< int, 8 >{} );
   [&]< int... Q >( std::integer_sequence< int, Q... > ) { ( p2_term< C, Q >( A, w, R, acc ), ... ); }
   ( std::make_integer_sequence< int, NQ >{} );
   acc         = A.alpha * acc;
   double* out = C == 0 ? A.dstV + i : A.dstE + edge_block_start( n, C ) + i;
   *out        = A.update == HYTEG_HIP_ADD ? *out + acc : acc;
}

// all eight destination kinds in one launch (blockIdx.y = kind): one ramp-up instead of eight, kinds overlap
__device__ inline void p2_inner_dispatch( const P2FastArgs& A, int kind )
{
   if ( !( ( A.kinds >> kind ) & 1u ) )
      return;
   switch ( kind )
   {
   case 0: p2_inner_body< 0 >( A ); break;
   case 1: p2_inner_body< 1 >( A ); break;
   case 2: p2_inner_body< 2 >( A ); break;
   case 3: p2_inner_body< 3 >( A ); break;
   case 4: p2_inner_body< 4 >( A ); break;
   case 5: p2_inner_body< 5 >( A ); break;
   case 6: p2_inner_body< 6 >( A ); break;
   default: p2_inner_body< 7 >( A ); break;
   }
}
__global__ __launch_bounds__( kThreads ) void p2_inner_kernel( const P2FastArgs A ) { p2_inner_dispatch( A, (int) blockIdx.y ); }
__global__ __launch_bounds__( kThreads ) void p2_inner_batch_kernel( const P2FastArgs F, const P2BatchPtrs P )
{
   const int cell = blockIdx.z;
   if ( !( P.mask[cell] & HYTEG_HIP_MASK_INNER ) )
      return;
   p2_inner_dispatch( p2_batch_view( F, P, cell ), (int) blockIdx.y );
}

// Boundary DoFs in stencil form (levels >= 2): which adjacent micro-cells exist depends only on the macro-primitive the DoF
// lies on, so every (destination kind, point class) has its own weight row over the SAME compile-time entry list; entries
// whose weight is zero (neighbour outside the macro-cell, or a genuinely vanishing coupling) are skipped.  Dense enumeration
// over the four faces of each kind's tetrahedral array as in p2_elementwise_kernel.
template < int C, int Q >
__device__ inline void p2_term_class( const P2FastArgs& A, const double* __restrict__ w, const RowBases& R, double& acc )
{
   constexpr int K = KindStencilOf< C >::value.kind[Q], DX = KindStencilOf< C >::value.dx[Q], DY = KindStencilOf< C >::value.dy[Q],
                 DZ = KindStencilOf< C >::value.dz[Q];
   // unconditional load from a safe index instead of a branch: all loads of a thread stay in flight together
   const double wq  = w[Q];
   const int    idx = wq != 0.0 ? R.b[K][DY + 1][DZ + 1] + DX : 0;
   acc              = fma( wq, K == 0 ? A.srcV[idx] : A.srcE[idx], acc );
}
struct P2ClassArgs
{
   P2FastArgs F;
   unsigned   mask;
};
template < int C >
__device__ inline void p2_boundary_body( const P2ClassArgs& B, int bx )
{
   constexpr int     NQ  = KindStencilOf< C >::value.n;
   constexpr int     OFF = class_offset( C );
   const P2FastArgs& A   = B.F;
   const int         N = A.N, n = N - 1;
   const int         W = C == 0 ? N : ( C == 7 ? n - 1 : n );
   if ( W <= 0 )
      return;
   const int T = tri( W );
   const int q = bx * kThreads + threadIdx.x;
   if ( q >= 4 * T )
      return;
   int x, y, z;
   {
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
   int cls;
   if constexpr ( C == 0 )
      cls = slot_from_flags< 14 >( z == 0, y == 0, x == 0, x + y + z == N - 1 );
   else
      cls = edge_class( N, x, y, z, C - 1 );
   if ( cls == 14 || !( ( B.mask >> cls ) & 1u ) )
      return;
   const double* __restrict__ w = A.table + OFF + cls * NQ;
   double   acc                 = 0.0;
   RowBases R;
   [&]< int... K >( std::integer_sequence< int, K... > ) { ( p2_row_bases_of_kind< C, K >( R, N, n, x, y, z ), ... ); }
   ( std::make_integer_sequence< int, 8 >{} );
   [&]< int... Q >( std::integer_sequence< int, Q... > ) { ( p2_term_class< C, Q >( A, w, R, acc ), ... ); }
   ( std::make_integer_sequence< int, NQ >{} );
   acc            = A.alpha * acc;
   const int i    = cell_index( W, x, y, z );
   double*   out  = C == 0 ? A.dstV + i : A.dstE + edge_block_start( n, C ) + i;
   *out           = A.update == HYTEG_HIP_ADD ? *out + acc : acc;
}
__device__ inline void p2_boundary_dispatch( const P2ClassArgs& B, int kind, int bx )
{
   if ( !( ( B.F.kinds >> kind ) & 1u ) )
      return;
   switch ( kind )
   {
   case 0: p2_boundary_body< 0 >( B, bx ); break;
   case 1: p2_boundary_body< 1 >( B, bx ); break;
   case 2: p2_boundary_body< 2 >( B, bx ); break;
   case 3: p2_boundary_body< 3 >( B, bx ); break;
   case 4: p2_boundary_body< 4 >( B, bx ); break;
   case 5: p2_boundary_body< 5 >( B, bx ); break;
   case 6: p2_boundary_body< 6 >( B, bx ); break;
   default: p2_boundary_body< 7 >( B, bx ); break;
   }
}
__global__ __launch_bounds__( kThreads ) void p2_boundary_kernel( const P2ClassArgs B ) { p2_boundary_dispatch( B, blockIdx.y, blockIdx.x ); }
__global__ __launch_bounds__( kThreads ) void p2_boundary_batch_kernel( const P2FastArgs F, const P2BatchPtrs P )
{
   const int      cell  = blockIdx.z;
   const unsigned shell = P.mask[cell] & HYTEG_HIP_MASK_SHELL;
   if ( shell == 0 )
      return;
   P2ClassArgs B;
   B.F    = p2_batch_view( F, P, cell );
   B.mask = shell;
   p2_boundary_dispatch( B, blockIdx.y, blockIdx.x );
}

} // namespace
