// Row kernel of the P2 apply with every point class (round 3; levels >= 3): p2_class_rows_kernel and its batched form; the default
// path of hyteg_hip_p2_elementwise_apply_cell[s]_kinds.  Builds on the source-row lists and lane shifts of kernels_p2_rows.hpp.
// Reference: none of its own -- a kernel of this project's design; the point classes are the macro-primitives whose DoFs the
// reference's P2ConstantOperator updates in its macro-vertex, -edge, -face and -cell kernels.
#pragma once

#include "kernels_p2_rows.hpp"

namespace {

// =====================================================================================================================
// Row kernel with every point class (round 3; levels >= 3, all destination kinds, masks that include the inner DoFs): replaces the
// launch of p2_rows_body_dpp + p2_boundary_body.  One wave owns a run of 62 positions of a row (y, z) of the vertex array (lanes
// 1..62; lanes 0 and 63 hold the x-neighbours), loads the 44 source rows once and produces all eight kinds, as p2_rows_body_dpp does.
// What is new:
//   * BOUNDARY DoFs are computed by the same waves.  The point class of a DoF -- which adjacent micro-cells exist -- depends on
//     four flags (z = 0, y = 0, x = 0, x + y + z = n; for an edge DoF: both end points).  The first two are wave-uniform, and within
//     a row only its FIRST DoF can have x = 0 and only its LAST one x + y + z = n.  So three passes, each with ONE class per wave and
//     therefore a wave-uniform weight row of the operator table (scalar loads, weights as SGPR operands): pass 0 all DoFs of the run
//     off those two planes, pass 1 the DoF at x = 0 (tiles with x0 = 0, the four kinds that can lie in that plane), pass 2 the last
//     DoF of the row (the tile that holds it, the four kinds that can lie on x + y + z = n).  Passes 1 and 2 run the whole wave for
//     one lane's DoF (138 FMAs each) -- far cheaper than the thread-per-DoF kernel, whose 65-96 loads per DoF hit a cache line each
//     on these two faces: level 7 (all DoFs) 44.4 -> 30.1 us, level 8 256 -> 156 us (profiles/r03_p2_class_rows.txt).
//   * The sum of a DoF runs in three partial sums (entries with dx = 0, +1, -1, each in the order of the entry list); the two
//     x-neighbour sums move by one lane at the end (two wave shifts per DoF instead of one per entry: 357 instead of 546 vector
//     instructions per wave, 99 VGPRs, 4 waves per SIMD).  Results agree with the other kernels to rounding, not bit for bit.
//   * Rows below y = 0 / z = 0 do not exist and are read as 0 (their base is moved beyond every array): the class weights of the
//     neighbours outside the macro-cell are exactly 0 and never meet a stray value.  Positions beyond the ends of a row (lane 0 of
//     the first tile, lanes past the last entry) read whatever the layout holds there, finite for finite input, and meet either a
//     zero weight or a lane that stores nothing -- as in p2_term_class, which reads entry 0 for its zero weights.
//
// Measured and not kept (same file): two positions per lane with 16-byte loads (NP = 2; range-checked dword by dword, so the half
// of a pair beyond the end of the array reads as 0): 196 VGPRs, slower at every level (level 7: 32.2 us inner DoFs against 25.0);
// a z-march (rows of slices z-1 .. z+2 in four register slots, 20 row loads per slice instead of 44): 184 VGPRs, 160 spilled
// SGPRs, 3.7 us per slice and wave, 40.7 us at level 7; the launch with every load and store forced out of range and no FMAs
// still takes 17 of 27 us -- the instruction stream of a wave, not the memory, is what these kernels are bound by.
// =====================================================================================================================
constexpr int      kClassRowsMinLevel = 3;
#ifndef HYTEG_P2_CLASS_ROWS_WAVES
#define HYTEG_P2_CLASS_ROWS_WAVES 4
#endif
constexpr int      kClassRowsWaves    = HYTEG_P2_CLASS_ROWS_WAVES; // waves per workgroup
#ifndef HYTEG_P2_DST_AUX
#define HYTEG_P2_DST_AUX 0
#endif
constexpr int      kClassRowsDstAux   = HYTEG_P2_DST_AUX; // cache policy of the destination arrays: 0 = plain; 2 = nontemporal measured: level 7 30.1 -> 29.1 us, level 8 156 -> 162, levels 4-5 +5 %
typedef int p2_v4i __attribute__( ( ext_vector_type( 4 ) ) );

template < int C >
struct DxUse
{
   bool plus, minus;
};
template < int C >
constexpr DxUse< C > build_dx_use()
{
   DxUse< C >            U{};
   constexpr KindStencil S = KindStencilOf< C >::value;
   for ( int q = 0; q < S.n; ++q )
   {
      U.plus  = U.plus || S.dx[q] > 0;
      U.minus = U.minus || S.dx[q] < 0;
   }
   return U;
}

// destination kind C at the NP positions xa .. xa + NP - 1 of row (y, z) a lane holds; R[row] = its NP source values in that row
// PASS 0: the DoFs off the planes x = 0 and x + y + z = n (one class per row: flags z == 0, y == 0).  PASS 1: the DoF at x = 0 of the row
// (kinds that can lie in that plane; tiles with x0 = 0).  PASS 2: the last DoF of the row, on x + y + z = n (kinds that can lie in that
// plane; the tile that holds it), unless it is the one at x = 0.  Every pass has ONE point class per wave, so its weights are a
// wave-uniform row of the operator table; passes 1 and 2 run the whole wave for one lane's DoF.
template < int C, int UPDATE, int NP, int PASS, bool RESTRICTED >
__device__ __forceinline__ void p2_classrows_kind( const P2RowsArgs& A, const double ( &R )[kRows.n][NP], const int ( &i0 )[3], int lane, int xa, int x0,
                                              int y, int z, unsigned mask, __amdgpu_buffer_rsrc_t rdV, __amdgpu_buffer_rsrc_t rdE )
{
   constexpr int  NQ = KindStencilOf< C >::value.n;
   constexpr bool F0 = C == 0 || C == 1 || C == 2 || C == 4; // kinds whose DoFs can lie in the plane z = 0 / y = 0 / x = 0 / x + y + z = n
   constexpr bool F1 = C == 0 || C == 1 || C == 3 || C == 5; // (both end points of the edge)
   constexpr bool F2 = C == 0 || C == 2 || C == 3 || C == 6;
   constexpr bool F3 = C == 0 || C == 4 || C == 5 || C == 6;
   if constexpr ( ( PASS == 1 && !F2 ) || ( PASS == 2 && !F3 ) )
      return;
   if ( RESTRICTED && !( ( A.F.kinds >> C ) & 1u ) ) // wave-uniform: a kind-restricted apply (the per-type sweeps of the P2 Gauss-Seidel smoother)
      return;
   const int  Nn = A.F.N, nn = Nn - 1;
   const int  top = ( C == 0 ? Nn - 1 : ( C == 7 ? nn - 2 : nn - 1 ) ) - y - z; // x of the last entry of the row in the kind's array
   const bool f0 = F0 && z == 0, f1 = F1 && y == 0;
   int        cls, xOnly = 0;
   if constexpr ( PASS == 0 )
      cls = f0 ? ( f1 ? 0 : 6 ) : ( f1 ? 7 : 14 );
   else if constexpr ( PASS == 1 )
   {
      if ( x0 != 0 || top < 0 )
         return;
      cls = slot_from_flags< 14 >( f0, f1, 1, F3 && top == 0 );
   }
   else
   {
      xOnly = top;
      if ( xOnly < ( F2 ? 1 : 0 ) || xOnly < x0 || xOnly >= x0 + 62 * NP )
         return;
      cls = slot_from_flags< 14 >( f0, f1, 0, 1 );
   }
   if ( !( ( mask >> cls ) & 1u ) ) // wave-uniform
      return;
   constexpr int OFF_INNER = stencil_offset( C ), OFF_CLASS = class_offset( C ); // forced constant evaluation (none of the table code on the device)
   const int     woff      = cls == 14 ? OFF_INNER : OFF_CLASS + cls * NQ;
   typedef const __attribute__( ( address_space( 4 ) ) ) double* cptr_t;
   const cptr_t w = (cptr_t) ( A.F.table + woff );
   double       a0[NP] = {}, ap[NP] = {}, am[NP] = {};
   [&]< int... Q >( std::integer_sequence< int, Q... > ) {
      ( ( [&] {
           constexpr int I   = SrcIndex< C >::value.idx[Q];
           constexpr int DX  = kSrc.dx[I];
           constexpr int row = kRows.ofSrc[I];
           const double  wq  = w[Q];
           for ( int p = 0; p < NP; ++p )
              if constexpr ( DX == 0 )
                 a0[p] = fma( wq, R[row][p], a0[p] );
              else if constexpr ( DX > 0 )
                 ap[p] = fma( wq, R[row][p], ap[p] );
              else
                 am[p] = fma( wq, R[row][p], am[p] );
        }() ),
        ... );
   }
   ( std::make_integer_sequence< int, NQ >{} );
   // position p takes the dx = +1 sum formed at position p + 1 and the dx = -1 sum formed at position p - 1 (in the next / previous lane
   // at the ends of the lane's run)
   constexpr DxUse< C > U = build_dx_use< C >();
   double               acc[NP];
   for ( int p = 0; p < NP; ++p )
      acc[p] = a0[p];
   if constexpr ( U.plus )
   {
      const double next = p2_lane_plus_1( ap[0] );
      for ( int p = 0; p < NP; ++p )
         acc[p] += p + 1 < NP ? ap[p + 1 < NP ? p + 1 : 0] : next;
   }
   if constexpr ( U.minus )
   {
      const double prev = p2_lane_minus_1( am[NP - 1] );
      for ( int p = 0; p < NP; ++p )
         acc[p] += p >= 1 ? am[p >= 1 ? p - 1 : 0] : prev;
   }
   const int     N  = A.F.N, n = N - 1;
   constexpr int c  = C == 0 ? 0 : ( C == 7 ? 2 : 1 );
   const int     bk = C == 0 ? 0 : ( C - 1 ) * (int) tet32( (unsigned) n );
   const __amdgpu_buffer_rsrc_t rd = C == 0 ? rdV : rdE;
   [&]< int... P >( std::integer_sequence< int, P... > ) {
      ( ( [&] {
           const int x = xa + P, s = x + y + z;
           // the DoF exists in its array and lies neither on x = 0 nor on x + y + z = n: p2_inner< C > without its conditions on y and z
           bool here;
           if constexpr ( C == 0 )
              here = x >= 1 && s <= N - 2;
           else if constexpr ( C == 1 )
              here = s < n;
           else if constexpr ( C == 2 || C == 3 )
              here = x > 0 && s < n;
           else if constexpr ( C == 6 )
              here = x > 0 && s < n - 1;
           else
              here = s < n - 1;
           bool on = lane >= 1 && lane <= 62;
           if constexpr ( PASS == 0 )
              on = on && here;
           else
              on = on && x == xOnly;
           const int  voff = on ? ( bk + i0[c] + NP * ( lane - 1 ) + P ) * 8 : -8;
           double     v    = A.F.alpha * acc[P];
           if constexpr ( UPDATE == HYTEG_HIP_ADD )
           {
              const p2_v2i o = __builtin_amdgcn_raw_buffer_load_b64( rd, voff, 0, kClassRowsDstAux );
              v              = __hiloint2double( o.y, o.x ) + v;
           }
           __builtin_amdgcn_raw_buffer_store_b64( p2_v2i{ __double2loint( v ), __double2hiint( v ) }, rd, voff, 0, kClassRowsDstAux );
        }() ),
        ... );
   }
   ( std::make_integer_sequence< int, NP >{} );
}

// RESTRICTED: only the destination kinds of A.F.kinds are computed and only the rows they read are loaded (the others' bases are moved
// beyond the arrays: the load is issued and returns 0 without touching memory)
template < int UPDATE, int NP, bool RESTRICTED = false >
__device__ __forceinline__ void p2_classrows_body( const P2RowsArgs& A, const Tile* tiles, int ntiles, int xcd_chunk, int block, unsigned mask )
{
   if ( xcd_chunk > 0 )
   {
      if ( ( block >> 3 ) >= xcd_chunk )
         return;
      block = ( block & 7 ) * xcd_chunk + ( block >> 3 );
   }
   const int t = __builtin_amdgcn_readfirstlane( block * kClassRowsWaves + ( (int) threadIdx.x >> 6 ) );
   if ( t >= ntiles )
      return;
   const Tile tl    = tiles[t]; // a, pad[0], pad[1]: index of (x0, y, z) at widths N, N-1, N-2; ya = y, yb = x0
   const int  lane  = threadIdx.x & 63;
   const int  N     = A.F.N;
   const int  y = tl.ya, z = tl.z, xa = tl.yb + NP * ( lane - 1 ); // lane 0 holds the NP positions in front of x0
   if ( !( mask & HYTEG_HIP_MASK_INNER ) )
   {
      // boundary classes only: a tile off the planes y = 0, z = 0 that holds neither the first nor (one of) the last entries of its rows
      // has nothing to compute
      const bool ends = tl.yb == 0 || tl.yb + 62 * NP > N - 2 - y - z;
      if ( !( mask & HYTEG_HIP_MASK_SHELL ) || !( ends || y == 0 || z == 0 ) )
         return;
   }
   const int  i0[3] = { tl.a, tl.pad[0], tl.pad[1] };
   const __amdgpu_buffer_rsrc_t rsV = __builtin_amdgcn_make_buffer_rsrc( const_cast< double* >( A.F.srcV ), 0, A.vbytes, 0x00020000 );
   const __amdgpu_buffer_rsrc_t rsE = __builtin_amdgcn_make_buffer_rsrc( const_cast< double* >( A.F.srcE ), 0, A.ebytes, 0x00020000 );
   const __amdgpu_buffer_rsrc_t rdV = __builtin_amdgcn_make_buffer_rsrc( A.F.dstV, 0, A.vbytes, 0x00020000 );
   const __amdgpu_buffer_rsrc_t rdE = __builtin_amdgcn_make_buffer_rsrc( A.F.dstE, 0, A.ebytes, 0x00020000 );
   const int  laneBytes = lane * 8 * NP;
   // rows below y = 0 / z = 0 do not exist: their base is moved beyond every array (two scalar flags, one select per such row); rows
   // beyond the top of a kind's array are read only by lanes whose results are not stored
   const bool rowBelow = y >= 1, sliceBelow = z >= 1;
   constexpr int kNowhere = (int) 0x80000000u;

   double R[kRows.n][NP];
   [&]< int... I >( std::integer_sequence< int, I... > ) {
      ( ( [&] {
           constexpr int K = kRows.kind[I], DY = kRows.dy[I], DZ = kRows.dz[I];
           int           base = p2_rows_base< K, DY, DZ >( i0, N, y, z ) + 8 - 8 * NP; // p2_rows_base is biased by one element
           if ( RESTRICTED && !( kRows.users[I] & A.F.kinds ) )
              base = kNowhere;
           if constexpr ( DY < 0 && DZ < 0 )
              base = ( rowBelow && sliceBelow ) ? base : kNowhere;
           else if constexpr ( DY < 0 )
              base = rowBelow ? base : kNowhere;
           else if constexpr ( DZ < 0 )
              base = sliceBelow ? base : kNowhere;
           if constexpr ( NP == 2 )
           {
              // a 16-byte load is range-checked dword by dword: the half of a pair that lies beyond the end of the array reads as 0
              const p2_v4i v = __builtin_amdgcn_raw_buffer_load_b128( K == 0 ? rsV : rsE, base + laneBytes, 0, 0 );
              R[I][0]        = __hiloint2double( v.y, v.x );
              R[I][NP - 1]   = __hiloint2double( v.w, v.z );
           }
           else
           {
              const p2_v2i v = __builtin_amdgcn_raw_buffer_load_b64( K == 0 ? rsV : rsE, base + laneBytes, 0, 0 );
              R[I][0]        = __hiloint2double( v.y, v.x );
           }
        }() ),
        ... );
   }
   ( std::make_integer_sequence< int, kRows.n >{} );

   [&]< int... C >( std::integer_sequence< int, C... > ) {
      ( p2_classrows_kind< C, UPDATE, NP, 0, RESTRICTED >( A, R, i0, lane, xa, tl.yb, y, z, mask, rdV, rdE ), ... );
      if ( mask & HYTEG_HIP_MASK_SHELL ) // wave-uniform: the DoFs on x = 0 and on x + y + z = n
      {
         ( p2_classrows_kind< C, UPDATE, NP, 1, RESTRICTED >( A, R, i0, lane, xa, tl.yb, y, z, mask, rdV, rdE ), ... );
         ( p2_classrows_kind< C, UPDATE, NP, 2, RESTRICTED >( A, R, i0, lane, xa, tl.yb, y, z, mask, rdV, rdE ), ... );
      }
   }
   ( std::make_integer_sequence< int, 8 >{} );
}

template < int UPDATE, int NP, bool RESTRICTED >
__global__ __launch_bounds__( 64 * kClassRowsWaves ) void p2_class_rows_kernel( const Tile* tiles, int ntiles, int xcd_chunk, const P2RowsArgs A, unsigned mask )
{
   p2_classrows_body< UPDATE, NP, RESTRICTED >( A, tiles, ntiles, xcd_chunk, (int) blockIdx.x, mask );
}

// the same for up to HYTEG_HIP_MAX_BATCH macro-cells of one level (blockIdx.y = cell), as p2_inner_batch_kernel
template < int UPDATE, bool RESTRICTED >
__global__ __launch_bounds__( 64 * kClassRowsWaves ) void p2_class_rows_batch_kernel( const Tile* tiles, int ntiles, const P2RowsArgs A, const P2BatchPtrs P )
{
   const int      cell = blockIdx.y;
   const unsigned mask = P.mask[cell];
   if ( mask == 0 )
      return;
   P2RowsArgs B = A;
   B.F          = p2_batch_view( A.F, P, cell );
   p2_classrows_body< UPDATE, 1, RESTRICTED >( B, tiles, ntiles, 0, (int) blockIdx.x, mask );
}

} // namespace
