// C-ABI entry point hyteg_hip_p1_cg_update_cells: the vector body of a conjugate gradient iteration in ONE pass.
// It replaces three host-layer calls of CGSolver::solve (src/hyteg/solvers/CGSolver.hpp:152-154)
//      x.add( { alpha }, { p } );   r.add( { -alpha }, { ap } );   rsnew = r.dotGlobal( r )
// i.e. the per-primitive loops of VertexDoFFunction::add (VertexDoFFunction.cpp:1408-1484) twice and of dotLocal (:1710-1793)
// once: four launches that read 2 + 2 + 1 arrays and write 2 (56 bytes per DoF), two of them only to reload what the previous one
// stored.  Here every entry of x, r, p, ap is read once and x, r are written once: 48 bytes per DoF.
// A streaming kernel in the manner of p1_vector.hip: one workgroup per tile of 1024 consecutive entries of one z-slice, four
// entries per thread, all 16 loads of a thread issued before the first use (the index decode that classifies the points runs
// while they are in flight), 8-byte coalesced accesses, nontemporal stores.  Fixed (cell, tile) -> workgroup assignment and fixed
// reduction trees: the sum does not depend on timing.  Reduction tail as in hyteg_hip_p1_dot_cells: few workgroups take tickets
// and the last one folds the partial sums, many leave that to a second launch of one workgroup.
#include "cell_geometry.hpp"

using namespace hyteg_hip;

namespace {

constexpr int kTile      = 1024;
constexpr int kThreads   = 256;
constexpr int kPer       = kTile / kThreads;
constexpr int kMaxB      = HYTEG_HIP_MAX_BATCH;
constexpr int kMaxBlocks = 1024; // partial sums: the workspace of hyteg_hip_dot_workspace_bytes() holds 1024 + 256 doubles
// Up to this many workgroups the tail is the ticket; above, a second launch.  Measured on the MI355X with both tails at every size
// (level-5 cells, full masks, us per call): 33 workgroups 7.2 (tickets) / 8.7 (two launches), 66: 7.3 / 8.6, 99: 6.2 / 6.8,
// 165: 7.1 / 6.5, 264: 8.5 / 6.6, 660: 13.5 / 7.9 -- a ticket costs ~11 ns, the second launch ~1 us; they cross between 99 and 165.
constexpr int kTicketBlocks = 128;

struct CgUpdateArgs
{
   // the cells with a non-zero mask, in the caller's order
   double*       x[kMaxB];
   double*       r[kMaxB];
   const double* p[kMaxB];
   const double* ap[kMaxB];
   unsigned      updateMask[kMaxB], dotMask[kMaxB];
   const Tile*   tiles;
   int           N, ntiles, ncells;
   double        alpha;
   double*       partial;
   double*       result;
   unsigned*     counter; // null: p1_cg_update_final_kernel reduces the partial sums
};

__global__ __launch_bounds__( kThreads ) void p1_cg_update_kernel( const CgUpdateArgs A )
{
   __shared__ double sh[kThreads / 64];
   double            acc   = 0.0;
   const int         total = A.ntiles * A.ncells;
   for ( int w = blockIdx.x; w < total; w += gridDim.x )
   {
      const int           cell = w / A.ntiles;
      const Tile          tl   = A.tiles[w - cell * A.ntiles];
      const unsigned      um = A.updateMask[cell], dm = A.dotMask[cell];
      double* const       x  = A.x[cell];
      double* const       r  = A.r[cell];
      const double* const p  = A.p[cell];
      const double* const ap = A.ap[cell];
      const int           W = A.N - tl.z, s0 = slice_start( A.N, tl.z );
      double              vx[kPer], vr[kPer], vp[kPer], va[kPer];
      int                 idx[kPer];
#pragma unroll
      for ( int u = 0; u < kPer; ++u )
      {
         const int e = (int) threadIdx.x + u * kThreads;
         idx[u]      = tl.a + ( e < tl.cnt ? e : tl.cnt - 1 ); // clamped: the loads are always legal, the stores are predicated
         vx[u]       = x[idx[u]];
         vr[u]       = r[idx[u]];
         vp[u]       = p[idx[u]];
         va[u]       = ap[idx[u]];
      }
      unsigned bit[kPer]; // the point's class as a bit of the point masks, 0 for a slot past the end of the tile
#pragma unroll
      for ( int u = 0; u < kPer; ++u )
      {
         const int j  = idx[u] - s0;
         const int y  = row_of( W, j );
         const int xx = j - row_start( W, y );
         bit[u]       = (int) threadIdx.x + u * kThreads < tl.cnt ? 1u << point_slot< 14 >( A.N, xx, y, tl.z ) : 0u;
      }
#pragma unroll
      for ( int u = 0; u < kPer; ++u )
      {
         const bool   upd = ( bit[u] & um ) != 0u;
         const double nx  = fma( A.alpha, vp[u], vx[u] );
         const double nr  = upd ? fma( -A.alpha, va[u], vr[u] ) : vr[u];
         if ( upd )
         {
            __builtin_nontemporal_store( nx, &x[idx[u]] );
            __builtin_nontemporal_store( nr, &r[idx[u]] );
         }
         acc = ( bit[u] & dm ) ? fma( nr, nr, acc ) : acc;
      }
   }
   const double s = block_sum< kThreads >( acc, sh );
   if ( A.counter == nullptr )
   {
      if ( threadIdx.x == 0 )
         A.partial[blockIdx.x] = s;
      return;
   }
   // the ticket of dot_finish (p1_vector.hip): the partial sum is written through to memory (agent scope: the XCDs do not share an
   // L2) and acknowledged before the ticket is drawn; no release fence, which would be an L2 write-back per workgroup
   __shared__ bool last;
   if ( threadIdx.x == 0 )
   {
      __hip_atomic_store( A.partial + blockIdx.x, s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT );
      asm volatile( "s_waitcnt vmcnt(0)" ::: "memory" );
      last = __hip_atomic_fetch_add( A.counter, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT ) == gridDim.x - 1;
   }
   __syncthreads();
   if ( !last )
      return;
   double sum = 0.0;
   for ( int k = threadIdx.x; k < (int) gridDim.x; k += kThreads )
      sum += __hip_atomic_load( A.partial + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT );
   __syncthreads(); // sh is reused
   const double grand = block_sum< kThreads >( sum, sh );
   if ( threadIdx.x == 0 )
   {
      *A.result = grand;
      __hip_atomic_store( A.counter, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT );
   }
}

// the same order of additions as the last workgroup above
__global__ __launch_bounds__( kThreads ) void p1_cg_update_final_kernel( const double* partial, int n, double* result )
{
   __shared__ double sh[kThreads / 64];
   double            acc = 0.0;
   for ( int k = threadIdx.x; k < n; k += kThreads )
      acc += partial[k];
   const double s = block_sum< kThreads >( acc, sh );
   if ( threadIdx.x == 0 )
      *result = s;
}

} // namespace

extern "C" {

HYTEG_HIP_API int hyteg_hip_p1_cg_update_cells( int                  ncells,
                                                double* const*       x,
                                                double* const*       r,
                                                const double* const* p,
                                                const double* const* ap,
                                                double               alpha,
                                                int                  level,
                                                const unsigned*      update_masks,
                                                const unsigned*      dot_masks,
                                                double*              result_dev,
                                                void*                workspace_dev,
                                                hyteg_hip_stream_t   stream )
{
   HH_REQUIRE( ncells >= 1 && ncells <= kMaxB, "p1_cg_update_cells: ncells must be 1..HYTEG_HIP_MAX_BATCH" );
   HH_REQUIRE( any_level_ok( level ), "p1_cg_update_cells: level out of range [0,11]" );
   HH_REQUIRE( x && r && p && ap && update_masks && dot_masks && result_dev && workspace_dev, "p1_cg_update_cells: null pointer" );
   CgUpdateArgs A{};
   for ( int c = 0; c < ncells; ++c )
   {
      HH_REQUIRE( x[c] && r[c] && p[c] && ap[c], "p1_cg_update_cells: null array of a cell" );
      HH_REQUIRE( x[c] != r[c] && x[c] != p[c] && x[c] != ap[c] && r[c] != p[c] && r[c] != ap[c],
                  "p1_cg_update_cells: x and r must not alias another array of the same cell" );
      const unsigned um = update_masks[c] & HYTEG_HIP_MASK_ALL, dm = dot_masks[c] & HYTEG_HIP_MASK_ALL;
      if ( ( um | dm ) == 0u )
         continue; // not touched
      const int k     = A.ncells++;
      A.x[k]          = x[c];
      A.r[k]          = r[c];
      A.p[k]          = p[c];
      A.ap[k]         = ap[c];
      A.updateMask[k] = um;
      A.dotMask[k]    = dm;
   }
   TileTable tt;
   int       rc = get_tiles( level, TILES_FULL, kTile, &tt );
   if ( rc != HYTEG_HIP_OK )
      return rc;
   A.tiles = tt.dev, A.N = ( 1 << level ) + 1, A.ntiles = tt.count, A.alpha = alpha;
   A.partial = static_cast< double* >( workspace_dev );
   A.result  = result_dev;
   const int total = tt.count * A.ncells;
   if ( total == 0 )
   {
      // nothing selected: the sum over no points
      hipLaunchKernelGGL( p1_cg_update_final_kernel, dim3( 1 ), dim3( kThreads ), 0, as_stream( stream ), A.partial, 0, result_dev );
      HH_CHECK_HIP( hipGetLastError() );
      return HYTEG_HIP_OK;
   }
   const int blocks = total < kMaxBlocks ? total : kMaxBlocks;
   if ( blocks <= kTicketBlocks )
   {
      rc = dot_counter( as_stream( stream ), &A.counter );
      if ( rc != HYTEG_HIP_OK )
         return rc;
      hipLaunchKernelGGL( p1_cg_update_kernel, dim3( blocks ), dim3( kThreads ), 0, as_stream( stream ), A );
   }
   else
   {
      A.counter = nullptr;
      hipLaunchKernelGGL( p1_cg_update_kernel, dim3( blocks ), dim3( kThreads ), 0, as_stream( stream ), A );
      hipLaunchKernelGGL( p1_cg_update_final_kernel, dim3( 1 ), dim3( kThreads ), 0, as_stream( stream ), A.partial, blocks, result_dev );
   }
   HH_CHECK_HIP( hipGetLastError() );
   return HYTEG_HIP_OK;
}

} // extern "C"
