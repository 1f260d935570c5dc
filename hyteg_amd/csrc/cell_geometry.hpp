// Geometry of a macro-cell that the P1 and P2 kernels share -- the macro-primitive slot of a point, the stencil offsets, the
// neighbour and axis tables of the linear grid transfer -- and the workgroup reductions of the dot products, one definition each.
#pragma once

#include <cfloat>

#include "common.hpp"

namespace hyteg_hip {

// ---- macro-primitive of a point -----------------------------------------------------------------------------------------
// Slot in { edge0..5, face0..3, vertex0..3 } of the macro-primitive a point lies on, from its four face flags (z == 0, y == 0,
// x == 0, x + y + z == N - 1; for an edge DoF: both end points on the face), src/hyteg/indexing/MacroCellIndexing.cpp:36-91.
// INNER is the value for a point inside the cell: -1 where the slot indexes a table of 14, 14 where it is a bit of a point mask.
// The ladder is a macro with two function bodies because the kernels' instructions are pinned: a point form that calls the flags
// form is simplified before it is inlined and ends as a differently ordered select chain in every P1 kernel.
#define HH_SLOT_LADDER( INNER )                            \
   const int cnt = f0 + f1 + f2 + f3;                      \
   if ( cnt == 0 )                                         \
      return INNER;                                        \
   if ( cnt == 1 )                                         \
      return 6 + ( f0 ? 0 : f1 ? 1 : f2 ? 2 : 3 );         \
   if ( cnt == 2 )                                         \
   {                                                       \
      if ( f0 )                                            \
         return f1 ? 0 : ( f2 ? 1 : 2 );                   \
      if ( f1 )                                            \
         return f2 ? 3 : 4;                                \
      return 5;                                            \
   }                                                       \
   if ( f0 && f1 && f2 )                                   \
      return 10;                                           \
   if ( f0 && f1 && f3 )                                   \
      return 11;                                           \
   if ( f0 && f2 && f3 )                                   \
      return 12;                                           \
   return 13;
template < int INNER >
__host__ __device__ inline int slot_from_flags( int f0, int f1, int f2, int f3 )
{
   HH_SLOT_LADDER( INNER )
}
template < int INNER >
__host__ __device__ inline int point_slot( int N, int x, int y, int z )
{
   const int f0 = ( z == 0 ), f1 = ( y == 0 ), f2 = ( x == 0 ), f3 = ( x + y + z == N - 1 );
   HH_SLOT_LADDER( INNER )
}
#undef HH_SLOT_LADDER

// ---- tables: one initialiser each, instantiated as a __constant__ array and / or a compile-time one (a __constant__ array
// cannot be initialised from another array) -----------------------------------------------------------------------------------
// the 15 stencil offsets in the C-ABI's weight order (std::map< indexing::Index > order: z, then y, then x)
#define HH_STENCIL_OFFSETS                                                                                                  \
   {                                                                                                                        \
      { 0, 0, -1 }, { 1, 0, -1 }, { -1, 1, -1 }, { 0, 1, -1 }, { 0, -1, 0 }, { 1, -1, 0 }, { -1, 0, 0 }, { 0, 0, 0 },       \
          { 1, 0, 0 }, { -1, 1, 0 }, { 0, 1, 0 }, { 0, -1, 1 }, { 1, -1, 1 }, { -1, 0, 1 }, { 0, 0, 1 }                     \
   }
static __constant__ int kStencilOffs[15][3] = HH_STENCIL_OFFSETS;
constexpr int           kStencilOffsC[15][3] = HH_STENCIL_OFFSETS;
#undef HH_STENCIL_OFFSETS

// the 14 fine neighbours of a coarse point, in the summation order of the restriction
#define HH_RESTRICT_NEIGHBOURS                                                                                              \
   {                                                                                                                        \
      { -1, 0, 0 }, { -1, 0, 1 }, { -1, 1, -1 }, { -1, 1, 0 }, { 0, -1, 0 }, { 0, -1, 1 }, { 0, 0, -1 }, { 0, 0, 1 },       \
          { 0, 1, -1 }, { 0, 1, 0 }, { 1, -1, 0 }, { 1, -1, 1 }, { 1, 0, -1 }, { 1, 0, 0 }                                  \
   }
static __constant__ int kNB14[14][3] = HH_RESTRICT_NEIGHBOURS;
constexpr int           kNB14C[14][3] = HH_RESTRICT_NEIGHBOURS;
#undef HH_RESTRICT_NEIGHBOURS

// prolongation: a fine point that is not a coarse point is the midpoint of exactly one of the 7 stencil axes, selected by its
// parity pattern x & 1 | ( y & 1 ) << 1 | ( z & 1 ) << 2; kLoFirst tells which end point the reference's scatter loop
// (lexicographic over coarse points) would have added first
static __constant__ int kAxis[8][3] = { { 0, 0, 0 }, { 1, 0, 0 }, { 0, 1, 0 }, { 1, -1, 0 }, { 0, 0, 1 }, { 1, 0, -1 }, { 0, 1, -1 }, { 1, -1, 1 } };
#define HH_LO_FIRST            \
   {                           \
      1, 1, 1, 0, 1, 0, 0, 1   \
   }
static __constant__ int kLoFirst[8] = HH_LO_FIRST;
constexpr bool          kLoFirstC[8] = HH_LO_FIRST; // for compile-time parities
#undef HH_LO_FIRST

// ---- reductions -----------------------------------------------------------------------------------------------------------
__device__ inline double wave_sum( double v )
{
#pragma unroll
   for ( int off = 32; off > 0; off >>= 1 )
      v += __shfl_down( v, off, 64 );
   return v;
}

// sum over a workgroup of THREADS threads, valid in thread 0; sh: THREADS / 64 doubles of LDS
template < int THREADS >
__device__ inline double block_sum( double v, double* sh )
{
   v = wave_sum( v );
   if ( ( threadIdx.x & 63 ) == 0 )
      sh[threadIdx.x >> 6] = v;
   __syncthreads();
   double r = 0.0;
   if ( threadIdx.x == 0 )
   {
#pragma unroll
      for ( int k = 0; k < THREADS / 64; ++k )
         r += sh[k];
   }
   return r;
}

// the same with the result in every thread, and safe to call again at once (sh may still be read from the previous call)
template < int THREADS >
__device__ inline double block_sum_all( double v, double* sh )
{
   v = wave_sum( v );
   __syncthreads();
   if ( ( threadIdx.x & 63 ) == 0 )
      sh[threadIdx.x >> 6] = v;
   __syncthreads();
   double r = 0.0;
#pragma unroll
   for ( int k = 0; k < THREADS / 64; ++k )
      r += sh[k];
   return r;
}

// the min / max siblings of wave_sum and block_sum (exact, so their order is free; NaN is outside the contract)
__device__ inline double wave_min( double v )
{
#pragma unroll
   for ( int off = 32; off > 0; off >>= 1 )
      v = fmin( v, __shfl_down( v, off, 64 ) );
   return v;
}
__device__ inline double wave_max( double v )
{
#pragma unroll
   for ( int off = 32; off > 0; off >>= 1 )
      v = fmax( v, __shfl_down( v, off, 64 ) );
   return v;
}
template < int THREADS >
__device__ inline double block_min( double v, double* sh )
{
   v = wave_min( v );
   if ( ( threadIdx.x & 63 ) == 0 )
      sh[threadIdx.x >> 6] = v;
   __syncthreads();
   double r = v;
   if ( threadIdx.x == 0 )
   {
#pragma unroll
      for ( int k = 1; k < THREADS / 64; ++k )
         r = fmin( r, sh[k] );
   }
   return r;
}
template < int THREADS >
__device__ inline double block_max( double v, double* sh )
{
   v = wave_max( v );
   if ( ( threadIdx.x & 63 ) == 0 )
      sh[threadIdx.x >> 6] = v;
   __syncthreads();
   double r = v;
   if ( threadIdx.x == 0 )
   {
#pragma unroll
      for ( int k = 1; k < THREADS / 64; ++k )
         r = fmax( r, sh[k] );
   }
   return r;
}

// ---- the statistics reduction (hyteg_hip_p1_reduce_cells, hyteg_hip_p2_edge_reduce_cells) ------------------------------------
// five accumulators per lane, in the order of HYTEG_HIP_REDUCE_*; the starting values are the reference's
// (VertexDoFFunction.cpp:1809, 1912, 1962, 2012) and what an empty selection returns
struct Stats
{
   double v[HYTEG_HIP_REDUCE_COUNT] = { 0.0, 0.0, DBL_MAX, -DBL_MAX, 0.0 };
};
// an entry that is not selected is replaced by the neutral element of each accumulator, never used in arithmetic
__device__ inline void stats_take( Stats& s, double x, bool selected )
{
   const double ax = fabs( x );
   s.v[HYTEG_HIP_REDUCE_SUM] += selected ? x : 0.0;
   s.v[HYTEG_HIP_REDUCE_SUM_ABS] += selected ? ax : 0.0;
   s.v[HYTEG_HIP_REDUCE_MIN]     = fmin( s.v[HYTEG_HIP_REDUCE_MIN], selected ? x : DBL_MAX );
   s.v[HYTEG_HIP_REDUCE_MAX]     = fmax( s.v[HYTEG_HIP_REDUCE_MAX], selected ? x : -DBL_MAX );
   s.v[HYTEG_HIP_REDUCE_MAX_ABS] = fmax( s.v[HYTEG_HIP_REDUCE_MAX_ABS], selected ? ax : 0.0 );
}
// partial statistics b (an array in the order of HYTEG_HIP_REDUCE_*, `stride` doubles apart) folded into a
__device__ inline void stats_merge( Stats& s, const double* b, int stride )
{
   s.v[HYTEG_HIP_REDUCE_SUM] += b[HYTEG_HIP_REDUCE_SUM * stride];
   s.v[HYTEG_HIP_REDUCE_SUM_ABS] += b[HYTEG_HIP_REDUCE_SUM_ABS * stride];
   s.v[HYTEG_HIP_REDUCE_MIN]     = fmin( s.v[HYTEG_HIP_REDUCE_MIN], b[HYTEG_HIP_REDUCE_MIN * stride] );
   s.v[HYTEG_HIP_REDUCE_MAX]     = fmax( s.v[HYTEG_HIP_REDUCE_MAX], b[HYTEG_HIP_REDUCE_MAX * stride] );
   s.v[HYTEG_HIP_REDUCE_MAX_ABS] = fmax( s.v[HYTEG_HIP_REDUCE_MAX_ABS], b[HYTEG_HIP_REDUCE_MAX_ABS * stride] );
}
// the statistics of a workgroup, valid in thread 0; sh: HYTEG_HIP_REDUCE_COUNT * THREADS / 64 doubles of LDS (fixed trees)
template < int THREADS >
__device__ inline Stats block_stats( const Stats& s, double* sh )
{
   constexpr int W = THREADS / 64;
   Stats         r;
   r.v[HYTEG_HIP_REDUCE_SUM]     = block_sum< THREADS >( s.v[HYTEG_HIP_REDUCE_SUM], sh + HYTEG_HIP_REDUCE_SUM * W );
   r.v[HYTEG_HIP_REDUCE_SUM_ABS] = block_sum< THREADS >( s.v[HYTEG_HIP_REDUCE_SUM_ABS], sh + HYTEG_HIP_REDUCE_SUM_ABS * W );
   r.v[HYTEG_HIP_REDUCE_MIN]     = block_min< THREADS >( s.v[HYTEG_HIP_REDUCE_MIN], sh + HYTEG_HIP_REDUCE_MIN * W );
   r.v[HYTEG_HIP_REDUCE_MAX]     = block_max< THREADS >( s.v[HYTEG_HIP_REDUCE_MAX], sh + HYTEG_HIP_REDUCE_MAX * W );
   r.v[HYTEG_HIP_REDUCE_MAX_ABS] = block_max< THREADS >( s.v[HYTEG_HIP_REDUCE_MAX_ABS], sh + HYTEG_HIP_REDUCE_MAX_ABS * W );
   return r;
}

// Workgroups per cell of the statistics reduction, from the number of 256-entry tiles of a cell's array alone (never from the
// number of cells in the launch: a cell's partial results and their order are then the same in every batch).  Up to
// kReduceSoloTiles tiles one workgroup walks the whole cell and writes the result, one launch; above that the tiles are dealt
// round robin to min( tiles, kReduceMaxGroups ) workgroups and reduce_finish folds each cell's partial results in a second launch.
constexpr int kReduceSoloTiles = 32, kReduceMaxGroups = 1024;
inline int    reduce_groups( int64_t tiles )
{
   return tiles <= kReduceSoloTiles ? 1 : (int) ( tiles < kReduceMaxGroups ? tiles : kReduceMaxGroups );
}
// results[c][q] = partial results [c][q][0 .. groups) of cell c folded in ascending order by one workgroup per cell (p1_batch.hip)
int reduce_finish( hipStream_t stream, const double* partial, int ncells, int groups, double* results );

// 1 / numNeighborCells from the counts of the C-ABI, which must be >= 1
inline int to_nnc14( const double* nnc, Nnc14* out, const char* who )
{
   for ( int k = 0; k < 14; ++k )
   {
      HH_REQUIRE( nnc[k] >= 1.0, std::string( who ) + ": neighbour-cell counts must be >= 1" );
      out->inv[k] = 1.0 / nnc[k];
   }
   return HYTEG_HIP_OK;
}

} // namespace hyteg_hip
