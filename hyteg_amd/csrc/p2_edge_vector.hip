// Vector operations and dot products on the edge-DoF array of a macro-cell, masked by point class and edge orientation, for one
// macro-cell and for a batch.
// Reference: EdgeDoFFunction::assign / add / dotLocal on a macro-cell (src/hyteg/edgedofspace/EdgeDoFFunction.cpp; generic loops in
// EdgeDoFMacroCell.hpp).
#include "p2_common.hpp"

namespace {

__device__ inline bool edge_entry( int n, int64_t i, int& x, int& y, int& z, int& o )
{
   const int64_t blk = tet64( n );
   o                 = (int) ( i / blk );
   if ( o > 6 )
      return false;
   const int     W = o == 6 ? n - 1 : n;
   const int64_t r = i - (int64_t) o * blk;
   if ( W <= 0 || r >= tet64( W ) )
      return false;
   z           = slice_of( W, r );
   const int j = (int) ( r - ( tet64( W ) - tet64( W - z ) ) );
   y           = row_of( W - z, j );
   x           = j - row_start( W - z, y );
   return true;
}

struct EdgeVecArgs
{
   double*       dst;
   const double* src[HYTEG_HIP_MAX_SRCS];
   double        c[HYTEG_HIP_MAX_SRCS];
   int64_t       size;
   int           N, nsrc, op; // 0 assign, 1 add, 2 mult, 3 set constant c[0]
   unsigned      mask;
   unsigned      kinds; // bit k (1..7): edge DoFs of orientation k - 1 take part
};
__global__ __launch_bounds__( kThreads ) void p2_edge_vector_kernel( const EdgeVecArgs A )
{
   const int64_t i = (int64_t) blockIdx.x * kThreads + threadIdx.x;
   int           x, y, z, o;
   if ( i >= A.size || !edge_entry( A.N - 1, i, x, y, z, o ) || !( ( A.kinds >> ( o + 1 ) ) & 1u ) ||
        !( ( A.mask >> edge_class( A.N, x, y, z, o ) ) & 1u ) )
      return;
   double tmp;
   if ( A.op == 3 )
      tmp = A.c[0];
   else if ( A.op == 2 )
   {
      tmp = A.src[0][i];
      for ( int k = 1; k < A.nsrc; ++k )
         tmp *= A.src[k][i];
   }
   else
   {
      tmp = A.c[0] * A.src[0][i];
      for ( int k = 1; k < A.nsrc; ++k )
         tmp += A.c[k] * A.src[k][i];
      if ( A.op == 1 )
         tmp = A.dst[i] + tmp;
   }
   A.dst[i] = tmp;
}

// the same for up to HYTEG_HIP_MAX_BATCH macro-cells in one launch (blockIdx.y = cell): at the small levels of a multigrid cycle a
// launch per (cell, operation) is pure launch latency -- a Taylor-Hood V(3,3) cycle on 24 cells issued 54,000 of them (round 3)
struct EdgeVecBatchArgs
{
   double*       dst[HYTEG_HIP_MAX_BATCH];
   const double* src[HYTEG_HIP_MAX_SRCS][HYTEG_HIP_MAX_BATCH];
   unsigned      mask[HYTEG_HIP_MAX_BATCH];
   double        c[HYTEG_HIP_MAX_SRCS];
   int64_t       size;
   int           N, nsrc, op;
   unsigned      kinds;
};
__global__ __launch_bounds__( kThreads ) void p2_edge_vector_batch_kernel( const EdgeVecBatchArgs A )
{
   const int      cell = blockIdx.y;
   const unsigned mask = A.mask[cell];
   const int64_t  i    = (int64_t) blockIdx.x * kThreads + threadIdx.x;
   int            x, y, z, o;
   if ( mask == 0 || i >= A.size || !edge_entry( A.N - 1, i, x, y, z, o ) || !( ( A.kinds >> ( o + 1 ) ) & 1u ) ||
        !( ( mask >> edge_class( A.N, x, y, z, o ) ) & 1u ) )
      return;
   double* dst = A.dst[cell];
   double  tmp;
   if ( A.op == 3 )
      tmp = A.c[0];
   else if ( A.op == 2 )
   {
      tmp = A.src[0][cell][i];
      for ( int k = 1; k < A.nsrc; ++k )
         tmp *= A.src[k][cell][i];
   }
   else
   {
      tmp = A.c[0] * A.src[0][cell][i];
      for ( int k = 1; k < A.nsrc; ++k )
         tmp += A.c[k] * A.src[k][cell][i];
      if ( A.op == 1 )
         tmp = dst[i] + tmp;
   }
   dst[i] = tmp;
}

constexpr int kEdgeDotBlocks = 1024;
__global__ __launch_bounds__( kThreads ) void p2_edge_dot_kernel( const double* __restrict__ a, const double* __restrict__ b, int64_t size, int N,
                                                                   unsigned mask, double* partial )
{
   __shared__ double sh[kThreads / 64];
   double            acc = 0.0;
   // fixed entry -> thread assignment: deterministic
   for ( int64_t i = (int64_t) blockIdx.x * kThreads + threadIdx.x; i < size; i += (int64_t) gridDim.x * kThreads )
   {
      int x, y, z, o;
      if ( edge_entry( N - 1, i, x, y, z, o ) && ( ( mask >> edge_class( N, x, y, z, o ) ) & 1u ) )
         acc = fma( a[i], b[i], acc );
   }
#pragma unroll
   for ( int off = 32; off > 0; off >>= 1 )
      acc += __shfl_down( acc, off, 64 );
   if ( ( threadIdx.x & 63 ) == 0 )
      sh[threadIdx.x >> 6] = acc;
   __syncthreads();
   if ( threadIdx.x == 0 )
   {
      double r = 0.0;
      for ( int k = 0; k < kThreads / 64; ++k )
         r += sh[k];
      partial[blockIdx.x] = r;
   }
}
// the masked dot product of up to HYTEG_HIP_MAX_BATCH macro-cells in one launch: one workgroup per cell walks the cell's edge-DoF array
// in a fixed order (deterministic); for the small levels of a cycle, where two launches per cell and dot product were 40 % of a
// Taylor-Hood cycle's kernel time (round 3)
struct EdgeDotBatchArgs
{
   const double* a[HYTEG_HIP_MAX_BATCH];
   const double* b[HYTEG_HIP_MAX_BATCH];
   unsigned      mask[HYTEG_HIP_MAX_BATCH];
   int64_t       size;
   int           N;
   double*       result; // [ncells]
};
__global__ __launch_bounds__( kThreads ) void p2_edge_dot_batch_kernel( const EdgeDotBatchArgs A )
{
   __shared__ double sh[kThreads / 64];
   const int         cell = blockIdx.x;
   const unsigned    mask = A.mask[cell];
   const double*     a    = A.a[cell];
   const double*     b    = A.b[cell];
   double            acc  = 0.0;
   if ( mask != 0 )
      for ( int64_t i = threadIdx.x; i < A.size; i += kThreads )
      {
         int x, y, z, o;
         if ( edge_entry( A.N - 1, i, x, y, z, o ) && ( ( mask >> edge_class( A.N, x, y, z, o ) ) & 1u ) )
            acc = fma( a[i], b[i], acc );
      }
#pragma unroll
   for ( int off = 32; off > 0; off >>= 1 )
      acc += __shfl_down( acc, off, 64 );
   if ( ( threadIdx.x & 63 ) == 0 )
      sh[threadIdx.x >> 6] = acc;
   __syncthreads();
   if ( threadIdx.x == 0 )
   {
      double r = 0.0;
      for ( int k = 0; k < kThreads / 64; ++k )
         r += sh[k];
      A.result[cell] = r;
   }
}
__global__ __launch_bounds__( kThreads ) void p2_sum_partials_kernel( const double* partial, int n, double* result )
{
   __shared__ double sh[kThreads / 64];
   double            acc = 0.0;
   for ( int k = threadIdx.x; k < n; k += kThreads )
      acc += partial[k];
#pragma unroll
   for ( int off = 32; off > 0; off >>= 1 )
      acc += __shfl_down( acc, off, 64 );
   if ( ( threadIdx.x & 63 ) == 0 )
      sh[threadIdx.x >> 6] = acc;
   __syncthreads();
   if ( threadIdx.x == 0 )
   {
      double r = 0.0;
      for ( int k = 0; k < kThreads / 64; ++k )
         r += sh[k];
      *result = r;
   }
}

// the statistics (sum, sum of magnitudes, min, max, max magnitude) of the edge-DoF arrays of up to HYTEG_HIP_MAX_BATCH macro-cells in one
// pass: blockIdx.y = cell, workgroup g of gridDim.x takes the 256-entry tiles g, g + gridDim.x, .. of the cell's array.  gridDim.x comes
// from the level alone (reduce_groups), so a cell's numbers do not depend on the batch it is in (batch_reduce_kernel, p1_batch.hip)
struct EdgeReduceArgs
{
   const double* a[HYTEG_HIP_MAX_BATCH];
   unsigned      mask[HYTEG_HIP_MAX_BATCH];
   int64_t       size;
   int           N;
   double*       partial; // [cell][statistic][workgroup of the cell]
   double*       results; // [cell][statistic]
};
__global__ __launch_bounds__( kThreads ) void p2_edge_reduce_batch_kernel( const EdgeReduceArgs A )
{
   __shared__ double sh[HYTEG_HIP_REDUCE_COUNT * kThreads / 64];
   const int         cell = blockIdx.y;
   const unsigned    mask = A.mask[cell];
   const double*     a    = A.a[cell];
   Stats             s;
   if ( mask != 0 )
      for ( int64_t i = (int64_t) blockIdx.x * kThreads + threadIdx.x; i < A.size; i += (int64_t) gridDim.x * kThreads )
      {
         int        x, y, z, o;
         const bool selected = edge_entry( A.N - 1, i, x, y, z, o ) && ( ( mask >> edge_class( A.N, x, y, z, o ) ) & 1u );
         stats_take( s, a[i], selected );
      }
   const Stats r = block_stats< kThreads >( s, sh );
   if ( threadIdx.x != 0 )
      return;
   if ( gridDim.x == 1 )
   {
#pragma unroll
      for ( int q = 0; q < HYTEG_HIP_REDUCE_COUNT; ++q )
         A.results[cell * HYTEG_HIP_REDUCE_COUNT + q] = r.v[q];
      return;
   }
#pragma unroll
   for ( int q = 0; q < HYTEG_HIP_REDUCE_COUNT; ++q )
      A.partial[( cell * HYTEG_HIP_REDUCE_COUNT + q ) * gridDim.x + blockIdx.x] = r.v[q];
}

} // namespace

extern "C" {

HYTEG_HIP_API int hyteg_hip_p2_edge_reduce_cells( int ncells, const double* const* a, int level, const unsigned* masks, double* results_dev,
                                                  void* workspace_dev, hyteg_hip_stream_t stream )
{
   HH_REQUIRE( a && masks && results_dev && workspace_dev, "p2_edge_reduce_cells: null pointer" );
   HH_REQUIRE( ncells >= 1 && ncells <= HYTEG_HIP_MAX_BATCH, "p2_edge_reduce_cells: 1 <= ncells <= HYTEG_HIP_MAX_BATCH" );
   HH_REQUIRE( level >= 0 && level <= HYTEG_HIP_P2_MAX_LEVEL, "p2_edge_reduce_cells: level out of range [0,9]" );
   EdgeReduceArgs A{};
   A.size = (int64_t) hyteg_hip_p2_edge_array_size( level ), A.N = ( 1 << level ) + 1;
   A.partial = static_cast< double* >( workspace_dev ), A.results = results_dev;
   for ( int c = 0; c < ncells; ++c )
   {
      HH_REQUIRE( a[c], "p2_edge_reduce_cells: null array" );
      A.a[c] = a[c], A.mask[c] = masks[c] & HYTEG_HIP_MASK_ALL;
   }
   const int groups = reduce_groups( ( A.size + kThreads - 1 ) / kThreads );
   hipLaunchKernelGGL( p2_edge_reduce_batch_kernel, dim3( (unsigned) groups, (unsigned) ncells ), dim3( kThreads ), 0, as_stream( stream ), A );
   HH_CHECK_HIP( hipGetLastError() );
   return groups == 1 ? HYTEG_HIP_OK : reduce_finish( as_stream( stream ), A.partial, ncells, groups, results_dev );
}

HYTEG_HIP_API int hyteg_hip_p2_edge_vector_cell_masked( int                  op,
                                                        double*              dst,
                                                        int                  nsrc,
                                                        const double* const* srcs,
                                                        const double*        scalars,
                                                        int                  level,
                                                        unsigned             mask,
                                                        hyteg_hip_stream_t   stream )
{
   return hyteg_hip_p2_edge_vector_cell_kinds( op, dst, nsrc, srcs, scalars, level, mask, 0xFEu, stream );
}

HYTEG_HIP_API int hyteg_hip_p2_edge_vector_cell_kinds( int                  op,
                                                       double*              dst,
                                                       int                  nsrc,
                                                       const double* const* srcs,
                                                       const double*        scalars,
                                                       int                  level,
                                                       unsigned             mask,
                                                       unsigned             kind_mask,
                                                       hyteg_hip_stream_t   stream )
{
   HH_REQUIRE( dst && op >= 0 && op <= 3, "p2_edge_vector_cell_masked: null dst or bad op" );
   HH_REQUIRE( level >= 0 && level <= HYTEG_HIP_P2_MAX_LEVEL, "p2_edge_vector_cell_masked: level out of range [0,9]" );
   HH_REQUIRE( op == 3 ? scalars != nullptr : ( nsrc >= 1 && nsrc <= HYTEG_HIP_MAX_SRCS && srcs ), "p2_edge_vector_cell_masked: bad sources" );
   HH_REQUIRE( op == 2 || scalars, "p2_edge_vector_cell_masked: null scalars" );
   if ( ( mask & HYTEG_HIP_MASK_ALL ) == 0 || ( kind_mask & 0xFEu ) == 0 )
      return HYTEG_HIP_OK;
   EdgeVecArgs A{};
   A.dst = dst, A.N = ( 1 << level ) + 1, A.nsrc = nsrc, A.op = op, A.mask = mask & HYTEG_HIP_MASK_ALL, A.kinds = kind_mask & 0xFEu;
   A.size = (int64_t) hyteg_hip_p2_edge_array_size( level );
   if ( op == 3 )
      A.c[0] = scalars[0];
   else
      for ( int k = 0; k < nsrc; ++k )
      {
         HH_REQUIRE( srcs[k], "p2_edge_vector_cell_masked: null source" );
         A.src[k] = srcs[k];
         A.c[k]   = scalars ? scalars[k] : 1.0;
      }
   if ( A.size == 0 )
      return HYTEG_HIP_OK;
   hipLaunchKernelGGL( p2_edge_vector_kernel, dim3( (unsigned) ( ( A.size + kThreads - 1 ) / kThreads ) ), dim3( kThreads ), 0,
                       as_stream( stream ), A );
   HH_CHECK_HIP( hipGetLastError() );
   return HYTEG_HIP_OK;
}

HYTEG_HIP_API int hyteg_hip_p2_edge_vector_cells_kinds( int op, int ncells, double* const* dst, int nsrc, const double* const* srcs,
                                                        const double* scalars, int level, const unsigned* masks, unsigned kind_mask,
                                                        hyteg_hip_stream_t stream )
{
   HH_REQUIRE( dst && masks && op >= 0 && op <= 3, "p2_edge_vector_cells_kinds: null pointer or bad op" );
   HH_REQUIRE( ncells >= 1 && ncells <= HYTEG_HIP_MAX_BATCH, "p2_edge_vector_cells_kinds: 1 <= ncells <= HYTEG_HIP_MAX_BATCH" );
   HH_REQUIRE( level >= 0 && level <= HYTEG_HIP_P2_MAX_LEVEL, "p2_edge_vector_cells_kinds: level out of range [0,9]" );
   HH_REQUIRE( op == 3 ? scalars != nullptr : ( nsrc >= 1 && nsrc <= HYTEG_HIP_MAX_SRCS && srcs ), "p2_edge_vector_cells_kinds: bad sources" );
   HH_REQUIRE( op == 2 || scalars, "p2_edge_vector_cells_kinds: null scalars" );
   if ( ( kind_mask & 0xFEu ) == 0 )
      return HYTEG_HIP_OK;
   EdgeVecBatchArgs A{};
   A.N = ( 1 << level ) + 1, A.nsrc = nsrc, A.op = op, A.kinds = kind_mask & 0xFEu;
   A.size = (int64_t) hyteg_hip_p2_edge_array_size( level );
   if ( A.size == 0 )
      return HYTEG_HIP_OK;
   bool any = false;
   for ( int c = 0; c < ncells; ++c )
   {
      HH_REQUIRE( dst[c], "p2_edge_vector_cells_kinds: null destination" );
      A.dst[c]  = dst[c];
      A.mask[c] = masks[c] & HYTEG_HIP_MASK_ALL;
      any       = any || A.mask[c] != 0;
   }
   if ( !any )
      return HYTEG_HIP_OK;
   if ( op == 3 )
      A.c[0] = scalars[0];
   else
      for ( int k = 0; k < nsrc; ++k )
      {
         A.c[k] = scalars ? scalars[k] : 1.0;
         for ( int c = 0; c < ncells; ++c )
         {
            HH_REQUIRE( srcs[(size_t) k * ncells + c], "p2_edge_vector_cells_kinds: null source" );
            A.src[k][c] = srcs[(size_t) k * ncells + c];
         }
      }
   hipLaunchKernelGGL( p2_edge_vector_batch_kernel, dim3( (unsigned) ( ( A.size + kThreads - 1 ) / kThreads ), (unsigned) ncells ), dim3( kThreads ), 0,
                       as_stream( stream ), A );
   HH_CHECK_HIP( hipGetLastError() );
   return HYTEG_HIP_OK;
}

HYTEG_HIP_API int hyteg_hip_p2_edge_dot_cells_masked( int ncells, const double* const* a, const double* const* b, int level, const unsigned* masks,
                                                      double* results_dev, hyteg_hip_stream_t stream )
{
   HH_REQUIRE( a && b && masks && results_dev, "p2_edge_dot_cells_masked: null pointer" );
   HH_REQUIRE( ncells >= 1 && ncells <= HYTEG_HIP_MAX_BATCH, "p2_edge_dot_cells_masked: 1 <= ncells <= HYTEG_HIP_MAX_BATCH" );
   HH_REQUIRE( level >= 0 && level <= HYTEG_HIP_P2_MAX_LEVEL, "p2_edge_dot_cells_masked: level out of range [0,9]" );
   EdgeDotBatchArgs A{};
   A.size = (int64_t) hyteg_hip_p2_edge_array_size( level ), A.N = ( 1 << level ) + 1, A.result = results_dev;
   for ( int c = 0; c < ncells; ++c )
   {
      HH_REQUIRE( a[c] && b[c], "p2_edge_dot_cells_masked: null array" );
      A.a[c] = a[c], A.b[c] = b[c], A.mask[c] = masks[c] & HYTEG_HIP_MASK_ALL;
   }
   hipLaunchKernelGGL( p2_edge_dot_batch_kernel, dim3( (unsigned) ncells ), dim3( kThreads ), 0, as_stream( stream ), A );
   HH_CHECK_HIP( hipGetLastError() );
   return HYTEG_HIP_OK;
}

HYTEG_HIP_API int hyteg_hip_p2_edge_dot_cell_masked( const double*      a,
                                                     const double*      b,
                                                     int                level,
                                                     unsigned           mask,
                                                     double*            result_dev,
                                                     void*              workspace_dev,
                                                     hyteg_hip_stream_t stream )
{
   HH_REQUIRE( a && b && result_dev && workspace_dev, "p2_edge_dot_cell_masked: null pointer" );
   HH_REQUIRE( level >= 0 && level <= HYTEG_HIP_P2_MAX_LEVEL, "p2_edge_dot_cell_masked: level out of range [0,9]" );
   const int64_t size   = (int64_t) hyteg_hip_p2_edge_array_size( level );
   int64_t       blocks = ( size + kThreads - 1 ) / kThreads;
   blocks               = blocks < 1 ? 1 : ( blocks > kEdgeDotBlocks ? kEdgeDotBlocks : blocks );
   double* partial      = static_cast< double* >( workspace_dev );
   hipLaunchKernelGGL( p2_edge_dot_kernel, dim3( (unsigned) blocks ), dim3( kThreads ), 0, as_stream( stream ), a, b, size, ( 1 << level ) + 1,
                       mask & HYTEG_HIP_MASK_ALL, partial );
   hipLaunchKernelGGL( p2_sum_partials_kernel, dim3( 1 ), dim3( kThreads ), 0, as_stream( stream ), partial, (int) blocks, result_dev );
   HH_CHECK_HIP( hipGetLastError() );
   return HYTEG_HIP_OK;
}

HYTEG_HIP_API size_t hyteg_hip_p2_edge_array_size( int level )
{
   if ( level < 0 || level > HYTEG_HIP_P2_MAX_LEVEL )
      return 0;
   const int64_t n = (int64_t) 1 << level;
   return (size_t) ( 6 * tet64( n ) + tet64( n - 1 ) );
}

} // extern "C"
