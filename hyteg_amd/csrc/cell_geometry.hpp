// Geometry of a macro-cell that the P1 and P2 kernels share -- the macro-primitive slot of a point, the stencil offsets, the
// neighbour and axis tables of the linear grid transfer -- and the workgroup reductions of the dot products, one definition each.
#pragma once

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
