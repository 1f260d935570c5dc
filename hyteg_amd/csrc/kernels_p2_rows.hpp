// Row kernels of the P2 apply for the inner DoFs (round 2; levels >= 3): p2_rows_body (every source loaded), p2_rows_body_dpp
// (every source row loaded once), p2_rows_kernel, and p2_apply_fused_kernel, which runs the thread-per-DoF boundary workgroups
// beside the row waves.  Same sums in the same order as kernels_p2_threads.hpp.
// Reference: none of its own -- the mapping of rows to waves is this project's; what is computed are the stencils of the reference's
// P2ConstantOperator macro-cell kernels, as in kernels_p2_threads.hpp.
#pragma once

#include "kernels_p2_threads.hpp"

namespace {

// =====================================================================================================================
// Row form of the inner stencils (levels >= 3).  p2_inner_kernel (kernels_p2_threads.hpp) spends ~90 % of its ~900 instructions per
// DoF on index arithmetic (decoding (x, y, z) from the flat index, eight array indices, 64-bit addresses).  Here ONE WAVE
// owns a run of <= 64 consecutive micro-vertex positions x of one row (y, z) -- a TILES_ROWS tile of the vertex array -- and
// produces ALL EIGHT destination kinds at those positions:
//   * y, z are wave-uniform, so every row base is scalar arithmetic: the index of (x0, y, z) in the three array widths
//     (N, N-1, N-2) comes with the tile, the nine neighbour rows (y+dy, z+dz) of each width are layout-algebra deltas;
//   * the union of the sources of all eight stencils (kSrc: distinct (kind, dx, dy, dz); 230 stencil entries share them) is
//     loaded ONCE into registers by buffer loads whose whole byte offset sits in the vector offset -- a row that does not
//     exist or a position beyond the end of a row gives an offset that is either out of range (the descriptor returns 0) or
//     inside the array (a wrong value that only lanes use whose result is not stored): no clamping, no faults;
//   * each destination kind sums its entries in the same order with the same FMAs as p2_inner_kernel (bit-identical
//     results) and stores where p2_inner< C > holds.
// =====================================================================================================================
struct SrcList
{
   int n;
   int kind[160], dx[160], dy[160], dz[160];
};
constexpr SrcList build_src_list()
{
   SrcList U{};
   for ( int c = 0; c < 8; ++c )
   {
      const KindStencil S = build_kind_stencil( c );
      for ( int q = 0; q < S.n; ++q )
      {
         bool found = false;
         for ( int i = 0; i < U.n; ++i )
            found = found || ( U.kind[i] == S.kind[q] && U.dx[i] == S.dx[q] && U.dy[i] == S.dy[q] && U.dz[i] == S.dz[q] );
         if ( !found )
         {
            U.kind[U.n] = S.kind[q], U.dx[U.n] = S.dx[q], U.dy[U.n] = S.dy[q], U.dz[U.n] = S.dz[q];
            ++U.n;
         }
      }
   }
   return U;
}
constexpr SrcList kSrc = build_src_list();
static_assert( kSrc.n <= 160, "source list" );
template < int C >
struct SrcIndexOf
{
   int idx[kMaxStencil];
};
template < int C >
constexpr SrcIndexOf< C > build_src_index()
{
   SrcIndexOf< C >       R{};
   constexpr KindStencil S = KindStencilOf< C >::value;
   for ( int q = 0; q < S.n; ++q )
      for ( int i = 0; i < kSrc.n; ++i )
         if ( kSrc.kind[i] == S.kind[q] && kSrc.dx[i] == S.dx[q] && kSrc.dy[i] == S.dy[q] && kSrc.dz[i] == S.dz[q] )
            R.idx[q] = i;
   return R;
}
template < int C >
struct SrcIndex
{
   static constexpr SrcIndexOf< C > value = build_src_index< C >();
};

// which destination kinds use source i (bit per kind): a kind-restricted apply (the per-type sweeps of the P2 Gauss-Seidel
// smoother) loads only the sources of the kinds it computes
struct SrcUsers
{
   unsigned m[160];
};
constexpr SrcUsers build_src_users()
{
   SrcUsers          R{};
   const KindStencil S8[8] = { KindStencilOf< 0 >::value, KindStencilOf< 1 >::value, KindStencilOf< 2 >::value, KindStencilOf< 3 >::value,
                               KindStencilOf< 4 >::value, KindStencilOf< 5 >::value, KindStencilOf< 6 >::value, KindStencilOf< 7 >::value };
   for ( int i = 0; i < kSrc.n; ++i )
      for ( int c = 0; c < 8; ++c )
         for ( int q = 0; q < S8[c].n; ++q )
            if ( kSrc.kind[i] == S8[c].kind[q] && kSrc.dx[i] == S8[c].dx[q] && kSrc.dy[i] == S8[c].dy[q] && kSrc.dz[i] == S8[c].dz[q] )
               R.m[i] |= 1u << c;
   return R;
}
constexpr SrcUsers kSrcUsers = build_src_users();

constexpr int kRowsWaves = 4;

typedef int p2_v2i __attribute__( ( ext_vector_type( 2 ) ) );

// byte offset (without the lane part, biased by -8 so that dx = -1, 0, 1 become the instruction offsets 0, 8, 16) of row
// (y + DY, z + DZ) of source kind K, from the tile's indices i0[width class] of (x0, y, z)
template < int K, int DY, int DZ >
__device__ inline int p2_rows_base( const int ( &i0 )[3], int N, int y, int z )
{
   constexpr int c  = K == 0 ? 0 : ( K == 7 ? 2 : 1 );
   const int     n  = N - 1;
   const int     W  = N - c;
   const int     bk = K == 0 ? 0 : ( K - 1 ) * (int) tet32( (unsigned) n );
   return ( bk + p2_neighbour_row< DY, DZ >( i0[c], W - z, y ) - 1 ) * 8;
}

template < int C, int UPDATE >
__device__ inline void p2_rows_kind( const P2RowsArgs& A, const double ( &U )[kSrc.n], const int ( &i0 )[3], int lane, int x, int y, int z,
                                     int cnt, __amdgpu_buffer_rsrc_t rdV, __amdgpu_buffer_rsrc_t rdE )
{
   constexpr int NQ  = KindStencilOf< C >::value.n;
   constexpr int OFF = stencil_offset( C );
   // constant address space: the weights are read by scalar loads and enter the FMAs as SGPR operands
   typedef const __attribute__( ( address_space( 4 ) ) ) double* cptr_t;
   const cptr_t w   = (cptr_t) ( A.F.table + OFF );
   double       acc = 0.0;
   [&]< int... Q >( std::integer_sequence< int, Q... > ) { ( ( acc = fma( w[Q], U[SrcIndex< C >::value.idx[Q]], acc ) ), ... ); }
   ( std::make_integer_sequence< int, NQ >{} );
   acc                 = A.F.alpha * acc;
   const int  N        = A.F.N, n = N - 1;
   constexpr int c     = C == 0 ? 0 : ( C == 7 ? 2 : 1 );
   const int  bk       = C == 0 ? 0 : ( C - 1 ) * (int) tet32( (unsigned) n );
   const bool on       = lane < cnt && p2_inner< C >( N, x, y, z );
   const int  voff     = on ? ( bk + i0[c] + lane ) * 8 : -8;
   const __amdgpu_buffer_rsrc_t rd = C == 0 ? rdV : rdE;
   if constexpr ( UPDATE == HYTEG_HIP_ADD ) // compile-time: a run-time branch made every kind wait for the previous kind's store
   {
      const p2_v2i o = __builtin_amdgcn_raw_buffer_load_b64( rd, voff, 0, 0 );
      acc            = __hiloint2double( o.y, o.x ) + acc;
   }
   __builtin_amdgcn_raw_buffer_store_b64( p2_v2i{ __double2loint( acc ), __double2hiint( acc ) }, rd, voff, 0, 0 );
}

// RESTRICTED: only some destination kinds are computed (A.F.kinds) and only their sources are loaded; the unrestricted form
// keeps its loads free of branches (with one wave-uniform branch per load the full apply was 16 % slower)
template < int UPDATE, bool RESTRICTED = false >
__device__ inline void p2_rows_body( const P2RowsArgs& A, const Tile* tiles, int ntiles, int xcd_chunk, int block )
{
   // Workgroups b, b + 8, ... run on the same XCD: they take consecutive row groups of ONE chunk of the cell, so that the
   // source rows neighbouring destination rows share (every source row serves ~7 destination rows) are found in that XCD's
   // L2 instead of being fetched by up to four L2s
   if ( xcd_chunk > 0 )
   {
      if ( ( block >> 3 ) >= xcd_chunk )
         return;
      block = ( block & 7 ) * xcd_chunk + ( block >> 3 );
   }
   const int t = __builtin_amdgcn_readfirstlane( block * kRowsWaves + ( (int) threadIdx.x >> 6 ) );
   if ( t >= ntiles )
      return;
   const Tile tl   = tiles[t];
   const int  lane = threadIdx.x & 63;
   const int  N    = A.F.N;
   const int  y = tl.ya, z = tl.z, x = tl.yb + lane;
   const int  i0[3] = { tl.a, tl.pad[0], tl.pad[1] };
   const __amdgpu_buffer_rsrc_t rsV = __builtin_amdgcn_make_buffer_rsrc( const_cast< double* >( A.F.srcV ), 0, A.vbytes, 0x00020000 );
   const __amdgpu_buffer_rsrc_t rsE = __builtin_amdgcn_make_buffer_rsrc( const_cast< double* >( A.F.srcE ), 0, A.ebytes, 0x00020000 );
   const __amdgpu_buffer_rsrc_t rdV = __builtin_amdgcn_make_buffer_rsrc( A.F.dstV, 0, A.vbytes, 0x00020000 );
   const __amdgpu_buffer_rsrc_t rdE = __builtin_amdgcn_make_buffer_rsrc( A.F.dstE, 0, A.ebytes, 0x00020000 );
   const int lane8 = lane * 8;

   double U[kSrc.n];
   [&]< int... I >( std::integer_sequence< int, I... > ) {
      ( ( [&] {
           constexpr int K = kSrc.kind[I], DX = kSrc.dx[I], DY = kSrc.dy[I], DZ = kSrc.dz[I];
           double        u = 0.0;
           if ( !RESTRICTED || ( kSrcUsers.m[I] & A.F.kinds ) ) // wave-uniform: sources of kinds that are not computed are not loaded
           {
              const int    voff = p2_rows_base< K, DY, DZ >( i0, N, y, z ) + lane8 + ( DX + 1 ) * 8;
              const p2_v2i v    = __builtin_amdgcn_raw_buffer_load_b64( K == 0 ? rsV : rsE, voff, 0, 0 );
              u                 = __hiloint2double( v.y, v.x );
           }
           U[I] = u;
        }() ),
        ... );
   }
   ( std::make_integer_sequence< int, kSrc.n >{} );

   [&]< int... C >( std::integer_sequence< int, C... > ) {
      ( ( ( !RESTRICTED || ( ( A.F.kinds >> C ) & 1u ) ) ? p2_rows_kind< C, UPDATE >( A, U, i0, lane, x, y, z, tl.cnt, rdV, rdE ) : (void) 0 ), ... );
   }
   ( std::make_integer_sequence< int, 8 >{} );
}
// ---- the same with each source ROW loaded once (round 2, after the counters: 1.0 M load instructions per level-7 launch at
// ~16 cycles each in the CU's address / L1 path are what p2_rows_body is bound by -- TCP_TOTAL_CACHE_ACCESSES 18.4 M,
// L1 hit rate 95 %, L1 -> L2 latency 260 cycles, 56 % of the wave cycles waiting for instructions).  The 89 sources are 44
// distinct rows (kind, dy, dz) read at dx = -1, 0, +1: a wave loads each row once, lane l holding x0 - 1 + l, and takes the
// x-neighbours from the neighbouring lanes (DPP wave shifts, as the P1 apply does); it produces 62 positions (lanes 1..62).
// Same sources at the same addresses, same FMA order: bit-identical to p2_rows_body.
struct RowList
{
   int      n;
   int      kind[64], dy[64], dz[64];
   unsigned users[64]; // destination kinds that read the row
   int      ofSrc[160]; // row of source i
};
constexpr RowList build_row_list()
{
   RowList R{};
   for ( int i = 0; i < kSrc.n; ++i )
   {
      int r = -1;
      for ( int k = 0; k < R.n; ++k )
         if ( R.kind[k] == kSrc.kind[i] && R.dy[k] == kSrc.dy[i] && R.dz[k] == kSrc.dz[i] )
            r = k;
      if ( r < 0 )
      {
         r         = R.n++;
         R.kind[r] = kSrc.kind[i], R.dy[r] = kSrc.dy[i], R.dz[r] = kSrc.dz[i];
      }
      R.users[r] |= kSrcUsers.m[i];
      R.ofSrc[i] = r;
   }
   return R;
}
constexpr RowList kRows = build_row_list();
static_assert( kRows.n <= 64, "row list" );

__device__ inline double p2_lane_minus_1( double v )
{
   int lo = __double2loint( v ), hi = __double2hiint( v );
   lo     = __builtin_amdgcn_mov_dpp( lo, 0x138, 0xf, 0xf, true ); // wave_shr:1
   hi     = __builtin_amdgcn_mov_dpp( hi, 0x138, 0xf, 0xf, true );
   return __hiloint2double( hi, lo );
}
__device__ inline double p2_lane_plus_1( double v )
{
   int lo = __double2loint( v ), hi = __double2hiint( v );
   lo     = __builtin_amdgcn_mov_dpp( lo, 0x130, 0xf, 0xf, true ); // wave_shl:1
   hi     = __builtin_amdgcn_mov_dpp( hi, 0x130, 0xf, 0xf, true );
   return __hiloint2double( hi, lo );
}

constexpr int kRowsDppCapacity = 62;

template < int C, int UPDATE >
__device__ inline void p2_rows_kind_dpp( const P2RowsArgs& A, const double ( &R )[kRows.n], const int ( &i0 )[3], int lane, int x, int y, int z,
                                         int cnt, __amdgpu_buffer_rsrc_t rdV, __amdgpu_buffer_rsrc_t rdE )
{
   constexpr int NQ  = KindStencilOf< C >::value.n;
   constexpr int OFF = stencil_offset( C );
   typedef const __attribute__( ( address_space( 4 ) ) ) double* cptr_t;
   const cptr_t w   = (cptr_t) ( A.F.table + OFF );
   double       acc = 0.0;
   [&]< int... Q >( std::integer_sequence< int, Q... > ) {
      ( ( [&] {
           constexpr int I  = SrcIndex< C >::value.idx[Q];
           constexpr int DX = kSrc.dx[I];
           const double  r  = R[kRows.ofSrc[I]];
           const double  u  = DX == 0 ? r : ( DX > 0 ? p2_lane_plus_1( r ) : p2_lane_minus_1( r ) );
           acc              = fma( w[Q], u, acc );
        }() ),
        ... );
   }
   ( std::make_integer_sequence< int, NQ >{} );
   acc                 = A.F.alpha * acc;
   const int  N        = A.F.N, n = N - 1;
   constexpr int c     = C == 0 ? 0 : ( C == 7 ? 2 : 1 );
   const int  bk       = C == 0 ? 0 : ( C - 1 ) * (int) tet32( (unsigned) n );
   const bool on       = lane >= 1 && lane <= cnt && p2_inner< C >( N, x, y, z );
   const int  voff     = on ? ( bk + i0[c] + lane - 1 ) * 8 : -8;
   const __amdgpu_buffer_rsrc_t rd = C == 0 ? rdV : rdE;
   if constexpr ( UPDATE == HYTEG_HIP_ADD )
   {
      const p2_v2i o = __builtin_amdgcn_raw_buffer_load_b64( rd, voff, 0, 0 );
      acc            = __hiloint2double( o.y, o.x ) + acc;
   }
   __builtin_amdgcn_raw_buffer_store_b64( p2_v2i{ __double2loint( acc ), __double2hiint( acc ) }, rd, voff, 0, 0 );
}

template < int UPDATE, bool RESTRICTED = false >
__device__ inline void p2_rows_body_dpp( const P2RowsArgs& A, const Tile* tiles, int ntiles, int xcd_chunk, int block )
{
   if ( xcd_chunk > 0 )
   {
      if ( ( block >> 3 ) >= xcd_chunk )
         return;
      block = ( block & 7 ) * xcd_chunk + ( block >> 3 );
   }
   const int t = __builtin_amdgcn_readfirstlane( block * kRowsWaves + ( (int) threadIdx.x >> 6 ) );
   if ( t >= ntiles )
      return;
   const Tile tl   = tiles[t]; // capacity 62
   const int  lane = threadIdx.x & 63;
   const int  N    = A.F.N;
   const int  y = tl.ya, z = tl.z, x = tl.yb - 1 + lane;
   const int  i0[3] = { tl.a, tl.pad[0], tl.pad[1] };
   const __amdgpu_buffer_rsrc_t rsV = __builtin_amdgcn_make_buffer_rsrc( const_cast< double* >( A.F.srcV ), 0, A.vbytes, 0x00020000 );
   const __amdgpu_buffer_rsrc_t rsE = __builtin_amdgcn_make_buffer_rsrc( const_cast< double* >( A.F.srcE ), 0, A.ebytes, 0x00020000 );
   const __amdgpu_buffer_rsrc_t rdV = __builtin_amdgcn_make_buffer_rsrc( A.F.dstV, 0, A.vbytes, 0x00020000 );
   const __amdgpu_buffer_rsrc_t rdE = __builtin_amdgcn_make_buffer_rsrc( A.F.dstE, 0, A.ebytes, 0x00020000 );
   const int lane8 = lane * 8;

   double R[kRows.n];
   [&]< int... I >( std::integer_sequence< int, I... > ) {
      ( ( [&] {
           constexpr int K = kRows.kind[I], DY = kRows.dy[I], DZ = kRows.dz[I];
           double        u = 0.0;
           if ( !RESTRICTED || ( kRows.users[I] & A.F.kinds ) )
           {
              // p2_rows_base is biased by one element: + lane8 addresses x0 - 1 + lane
              const int    voff = p2_rows_base< K, DY, DZ >( i0, N, y, z ) + lane8;
              const p2_v2i v    = __builtin_amdgcn_raw_buffer_load_b64( K == 0 ? rsV : rsE, voff, 0, 0 );
              u                 = __hiloint2double( v.y, v.x );
           }
           R[I] = u;
        }() ),
        ... );
   }
   ( std::make_integer_sequence< int, kRows.n >{} );

   [&]< int... C >( std::integer_sequence< int, C... > ) {
      ( ( ( !RESTRICTED || ( ( A.F.kinds >> C ) & 1u ) ) ? p2_rows_kind_dpp< C, UPDATE >( A, R, i0, lane, x, y, z, tl.cnt, rdV, rdE ) : (void) 0 ), ... );
   }
   ( std::make_integer_sequence< int, 8 >{} );
}

// the three values a wave needs before it can fetch its tile are leading scalar arguments: the command processor preloads them
// into SGPRs (-amdgpu-kernarg-preload-count=4), so the tile load does not wait for a kernel-argument load (as in the P1 apply;
// here without a measurable difference: 41.0 vs 40.7 us at level 7)
template < int UPDATE, bool RESTRICTED, bool DPP = false >
__global__ __launch_bounds__( 64 * kRowsWaves, 2 ) void p2_rows_kernel( const Tile* tiles, int ntiles, int xcd_chunk, const P2RowsArgs A )
{
   if constexpr ( DPP )
      p2_rows_body_dpp< UPDATE, RESTRICTED >( A, tiles, ntiles, xcd_chunk, (int) blockIdx.x );
   else
      p2_rows_body< UPDATE, RESTRICTED >( A, tiles, ntiles, xcd_chunk, (int) blockIdx.x );
}

// inner rows and boundary DoFs in ONE launch (they write disjoint DoFs and read the same sources): the boundary workgroups
// -- thread per DoF, a long chain of index arithmetic and dependent loads -- come first and run beside the row waves
// instead of after them
static_assert( kThreads == 64 * kRowsWaves, "the fused launch uses one block shape" );
template < int UPDATE, bool DPP = false >
__global__ __launch_bounds__( kThreads, 2 ) void p2_apply_fused_kernel( const Tile* tiles, int ntiles, int xcd_chunk, const P2RowsArgs A,
                                                                        unsigned shellMask, int nbx )
{
   if ( (int) blockIdx.x < 8 * nbx )
   {
      P2ClassArgs B;
      B.F    = A.F;
      B.mask = shellMask;
      p2_boundary_dispatch( B, (int) blockIdx.x / nbx, (int) blockIdx.x % nbx );
      return;
   }
   if constexpr ( DPP )
      p2_rows_body_dpp< UPDATE >( A, tiles, ntiles, xcd_chunk, (int) blockIdx.x - 8 * nbx );
   else
      p2_rows_body< UPDATE >( A, tiles, ntiles, xcd_chunk, (int) blockIdx.x - 8 * nbx );
}

} // namespace
