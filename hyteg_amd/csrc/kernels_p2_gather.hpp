// Table-driven micro-cell gather of the P2 elementwise operator (levels 0-1, where a DoF can be next to several macro-faces at
// once): p2_elementwise_kernel, one thread group per DoF, the adjacent micro-cells in the order the reference's scatter loop
// (P2ElementwiseOperator::localMatrixVectorMultiply3D, src/hyteg/elementwiseoperators/P2ElementwiseOperator.cpp:66-223) visits them.
#pragma once

#include <mutex>

#include "p2_common.hpp"

namespace {

struct LocalDof
{
   signed char kind; // 0 vertex array, 1..7 edge array block X, Y, Z, XY, XZ, YZ, XYZ
   signed char ox, oy, oz;
};
struct Entry
{
   signed char type, row, ox, oy, oz, pad[3];
};
struct P2Tables
{
   LocalDof    local[6][10];
   Entry       entries[8][24];
   signed char nentries[8];
};

struct P2Args
{
   double*       dstV;
   double*       dstE;
   const double* srcV;
   const double* srcE;
   const double* elmat; // device, [6][10][10]
   double        alpha;
   int           N, update;
   unsigned      mask;
   unsigned      kinds; // destination kinds to compute: bit 0 vertex DoFs, 1..7 edge DoFs X, Y, Z, XY, XZ, YZ, XYZ
   P2Tables      T;
};

// the tables, built once on the host: the local DoFs from c_local, and per destination kind the micro-cells that hold it
inline const P2Tables& tables()
{
   static P2Tables       T;
   static std::once_flag once;
   std::call_once( once, [] {
      for ( int t = 0; t < 6; ++t )
         for ( int k = 0; k < 10; ++k )
         {
            const CLocal l = c_local( t, k );
            T.local[t][k]  = LocalDof{ (signed char) l.kind, (signed char) l.ox, (signed char) l.oy, (signed char) l.oz };
         }
      for ( int c = 0; c < 8; ++c )
      {
         int n = 0;
         for ( int t = 0; t < 6; ++t )
         {
            // cells of one type contribute in micro-cell iteration order (z, y, x ascending), i.e. offsets descending
            int first = n;
            for ( int k = 0; k < 10; ++k )
               if ( T.local[t][k].kind == c )
                  T.entries[c][n++] = Entry{ (signed char) t, (signed char) k, T.local[t][k].ox, T.local[t][k].oy, T.local[t][k].oz, { 0, 0, 0 } };
            for ( int a = first; a < n; ++a )
               for ( int b = a + 1; b < n; ++b )
               {
                  const Entry &A = T.entries[c][a], &B = T.entries[c][b];
                  const bool   swap = B.oz > A.oz || ( B.oz == A.oz && ( B.oy > A.oy || ( B.oy == A.oy && B.ox > A.ox ) ) );
                  if ( swap )
                     std::swap( T.entries[c][a], T.entries[c][b] );
               }
         }
         T.nentries[c] = (signed char) n;
      }
   } );
   return T;
}

__constant__ int kRowDeficit[6]     = { 0, 1, 1, 2, 1, 1 }; // numCellsPerRowByType: n - deficit

// ---- the skeleton of a gather kernel, as device functions: the decode of a group index and the lane-group sum.  gather_kernel of
// kernels_p2_varcoef.hpp is built from them.  p2_elementwise_kernel below keeps its own copy of the same lines: built from these
// functions it computes the same but compiles to another instruction order (profiles/p2_varcoef_checks.txt). -------------------------
// group q as entry q of a tetrahedral array of width W; false: past its end
__device__ __forceinline__ bool p2_decode_all( int W, int q, int& x, int& y, int& z )
{
   if ( q >= (int) tet32( (unsigned) W ) )
      return false;
   z           = slice_of( W, q );
   const int j = q - slice_start( W, z );
   y           = row_of( W - z, j );
   x           = j - row_start( W - z, y );
   return true;
}
// group q of the boundary walk (see p2_elementwise_kernel): q -> face, ( i, j ), a point kept at its lowest-numbered face.  false: past
// the end, or a point that a lower face holds
__device__ __forceinline__ bool p2_decode_boundary( int W, int q, int& x, int& y, int& z )
{
   const int T = tri( W );
   if ( q >= 4 * T )
      return false;
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
   return lowest == f;
}
// The lane-group sum.  The G lanes of a DoF share its (at most 24) adjacent micro-cells, 24 / G each: lane l has evaluated entries
// l, l + G, l + 2 G, ... of the table into part[slot][NC], and vmask[slot] is the ballot of the lanes whose entry lies inside the
// macro-cell.  Every lane adds all contributions in the order of the table: one lane per DoF walks 24 dependent round trips (pure
// latency below level 7), G = 8 keeps three.  Every lane of a DoF's group must take part, or none.
template < int G, int NC >
__device__ __forceinline__ void p2_group_sum( const double ( &part )[24 / G][NC], const unsigned long long ( &vmask )[24 / G], double ( &acc )[NC] )
{
   const int base = ( threadIdx.x & 63 ) & ~( G - 1 ); // first lane of this DoF's group inside the wave
#pragma unroll
   for ( int l = 0; l < 24; ++l )
   {
      const bool on = ( vmask[l / G] >> ( base + ( l % G ) ) ) & 1ull;
#pragma unroll
      for ( int j = 0; j < NC; ++j )
      {
         const double p = __shfl( part[l / G][j], base + ( l % G ), 64 );
         if ( on )
            acc[j] += p;
      }
   }
}

// Boundary DoFs only, densely enumerated: the non-inner DoFs of a kind lie on faces of that kind's own tetrahedral array
// (all four for vertex DoFs, two for X .. YZ edge DoFs, none for XYZ), so thread q walks the four triangular faces
// (q -> face, (i,j)) and keeps a point at its lowest-numbered face.
template < int G >
__global__ __launch_bounds__( kThreads ) void p2_elementwise_kernel( const P2Args A )
{
   const int c = blockIdx.y; // destination kind
   const int N = A.N, n = N - 1;
   const int W = c == 0 ? N : ( c == 7 ? n - 1 : n );
   if ( W <= 0 || !( ( A.kinds >> c ) & 1u ) )
      return;
   // G lanes per DoF share its (at most 24) adjacent micro-cells, 24 / G each.  One thread per DoF walks 24 dependent memory
   // round trips: pure latency (39 us at level 5, 47 us at level 7); 32 lanes per DoF repeat the decode 32 times
   // (13 us at level 5 but 115 us at level 7); G = 8 keeps three round trips and a 8-fold decode.
   constexpr bool LANES = G > 1;
   const int      T     = tri( W );
   const int      lane  = threadIdx.x & ( G - 1 );
   const int      q     = blockIdx.x * ( kThreads / G ) + (int) threadIdx.x / G;
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
   const int64_t i = (int64_t) cell_index( W, x, y, z );
   int           cls;
   if ( c == 0 )
      cls = slot_from_flags< 14 >( z == 0, y == 0, x == 0, x + y + z == N - 1 );
   else
   {
      int f0 = 1, f1 = 1, f2 = 1, f3 = 1;
#pragma unroll
      for ( int e = 0; e < 2; ++e )
      {
         const int px = x + kEdgeEnds[c - 1][e][0], py = y + kEdgeEnds[c - 1][e][1], pz = z + kEdgeEnds[c - 1][e][2];
         f0 &= pz == 0, f1 &= py == 0, f2 &= px == 0, f3 &= px + py + pz == N - 1;
      }
      cls = slot_from_flags< 14 >( f0, f1, f2, f3 );
   }
   if ( !( ( A.mask >> cls ) & 1u ) )
      return;
   // one adjacent micro-cell: alpha * (row of its element matrix) . (its ten source values)
   auto contribution = [&]( int l, double& part ) -> bool {
      const Entry en = A.T.entries[c][l];
      const int   t = en.type, mx = x - en.ox, my = y - en.oy, mz = z - en.oz;
      const int   rows = n - kRowDeficit[t];
      if ( mx < 0 || my < 0 || mz < 0 || mx + my + mz > rows - 1 )
         return false;
      const double* M = A.elmat + 100 * t + 10 * en.row;
      double        s = 0.0;
#pragma unroll
      for ( int k = 0; k < 10; ++k )
      {
         const LocalDof ld = A.T.local[t][k];
         const int      px = mx + ld.ox, py = my + ld.oy, pz = mz + ld.oz;
         const double   v  = ld.kind == 0 ? A.srcV[(int64_t) cell_index( N, px, py, pz )] :
                                            A.srcE[edge_block_start( n, ld.kind ) + cell_index( ld.kind == 7 ? n - 1 : n, px, py, pz )];
         s                 = s + M[k] * v;
      }
      part = A.alpha * s;
      return true;
   };
   double acc = 0.0;
   if constexpr ( LANES )
   {
      // lane l evaluates micro-cells l, l + G, l + 2G, ...; every lane then adds all contributions in the reference's loop order
      constexpr int      kSlots = 24 / G;
      double             part[kSlots];
      unsigned long long vmask[kSlots];
#pragma unroll
      for ( int k = 0; k < kSlots; ++k )
      {
         part[k]          = 0.0;
         const int  l     = lane + k * G;
         const bool valid = l < A.T.nentries[c] && contribution( l, part[k] );
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
   }
   else
   {
      for ( int l = 0; l < A.T.nentries[c]; ++l )
      {
         double part;
         if ( contribution( l, part ) )
            acc += part;
      }
   }
   if ( lane != 0 )
      return;
   double* out = c == 0 ? A.dstV + i : A.dstE + edge_block_start( n, c ) + i;
   *out        = A.update == HYTEG_HIP_ADD ? *out + acc : acc;
}

} // namespace
