// What the P2 translation units share (p2_elementwise.hip, p2_edge_vector.hip, p2_constant_seam.hip, p2_sor_face.hip, p2_transfer.hip and the
// kernels_p2_*.hpp headers): index helpers of the P2 macro-cell arrays, the compile-time constant stencils of an affine macro-cell
// with the layout of the operator table, and the argument blocks of the apply kernels.
// Reference: celldof::macrocell::getMicroVerticesFromMicroCell (volumedofspace/CellDoFIndexing.hpp:155-198), edgedof::calcEdgeDoFIndex /
// calcEdgeDoFOrientation (edgedofspace/EdgeDoFIndexing.hpp:89-165), P2ConstantOperator's stencil maps.
// Everything sits in an anonymous namespace, as it did in the single file: every unit that includes this has its own copy, and the
// kernels keep their names.
#pragma once

#include <utility>

#include "cell_geometry.hpp"

using namespace hyteg_hip;

namespace {

constexpr int kThreads = 256;

// slice z of entry i of a tetrahedral array of width W (largest z with slice_start(W,z) <= i): cube-root estimate + fix-up
// (a binary search with 64-bit products was a quarter of the instructions of the inner kernels)
__device__ inline int slice_of( int W, int64_t i )
{
   const int64_t rest = tet64( W ) - i; // entries from i to the end: tet(W - z) >= rest > tet(W - z - 1)
   int           m    = (int) cbrtf( 6.0f * (float) rest );
   m                  = m < 1 ? 1 : ( m > W ? W : m );
   while ( m > 1 && tet64( m - 1 ) >= rest )
      --m;
   while ( tet64( m ) < rest )
      ++m;
   return W - m;
}

// the same in 32-bit arithmetic, for arrays below 2^31 entries (the P2 grid transfer: 64-bit products were a large part of its index decoding)
__device__ inline int slice_of( int W, int i )
{
   const unsigned rest = tet32( (unsigned) W ) - (unsigned) i;
   int            m    = (int) cbrtf( 6.0f * (float) rest );
   m                   = m < 1 ? 1 : ( m > W ? W : m );
   while ( m > 1 && tet32( (unsigned) ( m - 1 ) ) >= rest )
      --m;
   while ( tet32( (unsigned) m ) < rest )
      ++m;
   return W - m;
}

// end points of an edge DoF relative to its logical index, by orientation X, Y, Z, XY, XZ, YZ, XYZ
// (one initialiser for the device table and its host copy: a __constant__ array cannot be initialised from another array)
#define P2_EDGE_ENDS                                                                                                          \
   {                                                                                                                          \
      { { 0, 0, 0 }, { 1, 0, 0 } }, { { 0, 0, 0 }, { 0, 1, 0 } }, { { 0, 0, 0 }, { 0, 0, 1 } }, { { 1, 0, 0 }, { 0, 1, 0 } }, \
          { { 1, 0, 0 }, { 0, 0, 1 } }, { { 0, 1, 0 }, { 0, 0, 1 } }, { { 0, 1, 0 }, { 1, 0, 1 } }                             \
   }
__constant__ int kEdgeEnds[7][2][3]     = P2_EDGE_ENDS;
constexpr int    kEdgeEndsHost[7][2][3] = P2_EDGE_ENDS; // the same on the host
#undef P2_EDGE_ENDS

__device__ inline int64_t edge_block_start( int n, int kind ) { return (int64_t) ( kind - 1 ) * tet64( n ); }
__device__ inline int edge_class( int N, int x, int y, int z, int o )
{
   int f0 = 1, f1 = 1, f2 = 1, f3 = 1;
#pragma unroll
   for ( int e = 0; e < 2; ++e )
   {
      const int px = x + kEdgeEnds[o][e][0], py = y + kEdgeEnds[o][e][1], pz = z + kEdgeEnds[o][e][2];
      f0 &= pz == 0, f1 &= py == 0, f2 &= px == 0, f3 &= px + py + pz == N - 1;
   }
   return slot_from_flags< 14 >( f0, f1, f2, f3 );
}

// =====================================================================================================================
// Fast path for INNER DoFs: on an affine macro-cell every inner DoF of one kind sees the same neighbourhood, so the sum
// over its adjacent micro-cells collapses to a constant stencil  sum_q w[q] * src_{kind_q}( dof + d_q )  (what the reference's
// P2ConstantOperator assembles into its vertex-to-vertex, edge-to-vertex, vertex-to-edge and edge-to-edge stencils).  The list
// of (source kind, offset) pairs per destination kind is a geometric fact and is built at COMPILE time from the micro-cell
// tables, so the kernel is straight-line code with constant offsets; the weights are summed from the element matrices on
// the host (hyteg_hip_p2_build_operator_table) and read through scalar loads.
// =====================================================================================================================
struct CLocal
{
   int kind, ox, oy, oz;
};
constexpr int cMicroVerts[6][4][3] = { { { 0, 0, 0 }, { 1, 0, 0 }, { 0, 1, 0 }, { 0, 0, 1 } }, { { 1, 0, 0 }, { 1, 1, 0 }, { 0, 1, 0 }, { 1, 0, 1 } },
                                       { { 1, 0, 0 }, { 0, 1, 0 }, { 1, 0, 1 }, { 0, 0, 1 } }, { { 1, 1, 0 }, { 1, 1, 1 }, { 0, 1, 1 }, { 1, 0, 1 } },
                                       { { 1, 0, 1 }, { 0, 1, 1 }, { 0, 0, 1 }, { 0, 1, 0 } }, { { 0, 1, 0 }, { 1, 1, 0 }, { 1, 0, 1 }, { 0, 1, 1 } } };
constexpr int cEdgePairs[6][2]      = { { 2, 3 }, { 1, 3 }, { 1, 2 }, { 0, 3 }, { 0, 2 }, { 0, 1 } };

constexpr CLocal c_local( int t, int k )
{
   if ( k < 4 )
      return CLocal{ 0, cMicroVerts[t][k][0], cMicroVerts[t][k][1], cMicroVerts[t][k][2] };
   const int* a = cMicroVerts[t][cEdgePairs[k - 4][0]];
   const int* b = cMicroVerts[t][cEdgePairs[k - 4][1]];
   const int  d0 = b[0] - a[0], d1 = b[1] - a[1], d2 = b[2] - a[2];
   if ( d1 == 0 && d2 == 0 )
   {
      const int* lo = a[0] < b[0] ? a : b;
      return CLocal{ 1, lo[0], lo[1], lo[2] };
   }
   if ( d0 == 0 && d2 == 0 )
   {
      const int* lo = a[1] < b[1] ? a : b;
      return CLocal{ 2, lo[0], lo[1], lo[2] };
   }
   if ( d0 == 0 && d1 == 0 )
   {
      const int* lo = a[2] < b[2] ? a : b;
      return CLocal{ 3, lo[0], lo[1], lo[2] };
   }
   if ( d2 == 0 )
   {
      const int* lo = a[0] < b[0] ? a : b;
      return CLocal{ 4, lo[0], lo[1] - 1, lo[2] };
   }
   if ( d1 == 0 )
   {
      const int* lo = a[0] < b[0] ? a : b;
      return CLocal{ 5, lo[0], lo[1], lo[2] - 1 };
   }
   if ( d0 == 0 )
   {
      const int* lo = a[1] < b[1] ? a : b;
      return CLocal{ 6, lo[0], lo[1], lo[2] - 1 };
   }
   const int* lo = a[0] < b[0] ? a : b;
   return CLocal{ 7, lo[0], lo[1] - 1, lo[2] };
}

constexpr int kMaxStencil = 96;
struct KindStencil
{
   int n;
   int kind[kMaxStencil], dx[kMaxStencil], dy[kMaxStencil], dz[kMaxStencil];
};
// unique (source kind, offset) pairs of destination kind c, in first-seen order over (type, local row, local column)
constexpr KindStencil build_kind_stencil( int c )
{
   KindStencil S{};
   for ( int t = 0; t < 6; ++t )
      for ( int k = 0; k < 10; ++k )
      {
         const CLocal row = c_local( t, k );
         if ( row.kind != c )
            continue;
         for ( int j = 0; j < 10; ++j )
         {
            const CLocal col = c_local( t, j );
            const int    dx = col.ox - row.ox, dy = col.oy - row.oy, dz = col.oz - row.oz;
            bool         found = false;
            for ( int q = 0; q < S.n; ++q )
               found = found || ( S.kind[q] == col.kind && S.dx[q] == dx && S.dy[q] == dy && S.dz[q] == dz );
            if ( !found )
            {
               S.kind[S.n] = col.kind, S.dx[S.n] = dx, S.dy[S.n] = dy, S.dz[S.n] = dz;
               ++S.n;
            }
         }
      }
   return S;
}
template < int C >
struct KindStencilOf
{
   static constexpr KindStencil value = build_kind_stencil( C );
};
constexpr int stencil_count( int c ) { return build_kind_stencil( c ).n; }
constexpr int stencil_offset( int c )
{
   int o = 600; // the element matrices come first in the operator table
   for ( int k = 0; k < c; ++k )
      o += stencil_count( k );
   return o;
}
// after the inner stencils: per destination kind, 14 boundary point classes x the same entry list (weights of neighbours
// whose micro-cells do not exist for that class are exactly zero)
constexpr int class_offset( int c )
{
   int o = stencil_offset( 8 );
   for ( int k = 0; k < c; ++k )
      o += 14 * stencil_count( k );
   return o;
}
constexpr int kOperatorTableSize = class_offset( 8 );

struct P2FastArgs
{
   double*       dstV;
   double*       dstE;
   const double* srcV;
   const double* srcE;
   const double* table; // device: [600 element matrices | stencil weights of kind 0 | kind 1 | ... ]
   double        alpha;
   int           N, update;
   unsigned      kinds; // destination kinds to compute (bit per kind), as in P2Args
};

// the same for up to HYTEG_HIP_MAX_BATCH macro-cells of one level (blockIdx.z = cell): the cells' arrays, operator tables and point
// masks travel as pointer lists in the kernel arguments
struct P2BatchPtrs
{
   double*       dstV[HYTEG_HIP_MAX_BATCH];
   double*       dstE[HYTEG_HIP_MAX_BATCH];
   const double* srcV[HYTEG_HIP_MAX_BATCH];
   const double* srcE[HYTEG_HIP_MAX_BATCH];
   const double* table[HYTEG_HIP_MAX_BATCH];
   unsigned      mask[HYTEG_HIP_MAX_BATCH];
};
__device__ inline P2FastArgs p2_batch_view( const P2FastArgs& F, const P2BatchPtrs& P, int cell )
{
   P2FastArgs A = F;
   A.dstV = P.dstV[cell], A.dstE = P.dstE[cell], A.srcV = P.srcV[cell], A.srcE = P.srcE[cell], A.table = P.table[cell];
   return A;
}

struct P2RowsArgs
{
   P2FastArgs  F;
   const Tile* tiles; // TILES_ROWS of the vertex array, capacity 64; pad[0], pad[1] = the tile's first index at widths N-1, N-2
   int         ntiles;
   unsigned    vbytes, ebytes; // sizes of the vertex- and edge-DoF arrays
   int         xcd_chunk;      // row blocks per XCD: block b works on chunk b % 8 (0: blocks in launch order)
};

} // namespace
