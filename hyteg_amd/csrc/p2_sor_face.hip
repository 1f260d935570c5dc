// ---- Gauss-Seidel / SOR on the macro-edges and macro-faces shared between macro-cells, in the reference's order ------------------
// P2ConstantOperator::smooth_sor (src/constant_stencil_operator/P2ConstantOperator.cpp:1267-1330) sweeps macro-vertices, -edges,
// -faces, -cells one class after the other; a primitive's sweep sees current values on itself and its boundary and ghost-layer
// values for everything else.  Cell-centric form (as for P1, p1_sor_shell.hip): the ghost-layer part of every row is ONE apply
// with the operator table whose weights for sources ON the primitive's closure are zeroed (summed over the cells by the additive
// exchange); the closure part is evaluated with the complementary tables, and the only sequential piece -- the edge DoFs inside
// a macro-face, which couple with each other -- is swept on every cell's copy with the total weights by p2_sor_face_edges_kernel and its
// LDS forms in this file.
#include "p2_common.hpp"

namespace {
// a macro-face in the cell's index space: its vertices in the order of their global ids are the cell-local vertices l0, l1, l2;
// micro-vertex (i, j) of the face = O + i a + j b; edge DoF types of the face: X (i,j)-(i+1,j), XY (i+1,j)-(i,j+1), Y (i,j)-(i,j+1)
struct P2FaceFrame
{
   int    O[3], a[3], b[3]; // O is filled per level (n * unit vector of l0)
   int    kind[3];          // cell edge-DoF kind (1..6) of the face types X, XY, Y
   int    off[3][3];        // logical index of face edge (t, i, j) in the cell = O + i a + j b + off[t]
   double w[3][5];          // diagonal, then the four in-face neighbours of kFaceNb
};
// in-face neighbours of an edge DoF: (type, di, dj), the other edges of the two face triangles that share it
#define P2_FACE_NB                                                                                                            \
   {                                                                                                                         \
      { { 1, 0, 0 }, { 2, 0, 0 }, { 1, 0, -1 }, { 2, 1, -1 } }, { { 0, 0, 0 }, { 2, 0, 0 }, { 0, 0, 1 }, { 2, 1, 0 } },       \
      {                                                                                                                      \
         { 0, 0, 0 }, { 1, 0, 0 }, { 0, -1, 1 }, { 1, -1, 0 }                                                                \
      }                                                                                                                      \
   }
const int        kFaceNbHost[3][4][3] = P2_FACE_NB;
__constant__ int kFaceNb[3][4][3]     = P2_FACE_NB;
#undef P2_FACE_NB
bool face_frame( const int lv[3], P2FaceFrame& F, int& faceClass )
{
   static const int unit[4][3] = { { 0, 0, 0 }, { 1, 0, 0 }, { 0, 1, 0 }, { 0, 0, 1 } };
   static const int dirs[6][3] = { { 1, 0, 0 }, { 0, 1, 0 }, { 0, 0, 1 }, { -1, 1, 0 }, { -1, 0, 1 }, { 0, -1, 1 } };
   static const int e0[6][3]   = { { 0, 0, 0 }, { 0, 0, 0 }, { 0, 0, 0 }, { 1, 0, 0 }, { 1, 0, 0 }, { 0, 1, 0 } };
   for ( int k = 0; k < 3; ++k )
      if ( lv[k] < 0 || lv[k] > 3 )
         return false;
   if ( lv[0] == lv[1] || lv[0] == lv[2] || lv[1] == lv[2] )
      return false;
   const int missing = 6 - lv[0] - lv[1] - lv[2];
   faceClass         = 6 + ( missing == 3 ? 0 : ( missing == 2 ? 1 : ( missing == 1 ? 2 : 3 ) ) );
   for ( int r = 0; r < 3; ++r )
   {
      F.O[r] = unit[lv[0]][r]; // scaled by n by the caller
      F.a[r] = unit[lv[1]][r] - unit[lv[0]][r];
      F.b[r] = unit[lv[2]][r] - unit[lv[0]][r];
   }
   for ( int t = 0; t < 3; ++t )
   {
      int D[3], S[3]; // direction and start point (relative to micro-vertex (i, j)) of face type t
      for ( int r = 0; r < 3; ++r )
      {
         D[r] = t == 0 ? F.a[r] : ( t == 1 ? F.b[r] - F.a[r] : F.b[r] );
         S[r] = t == 1 ? F.a[r] : 0;
      }
      F.kind[t] = 0;
      for ( int k = 0; k < 6; ++k )
      {
         const bool plus  = D[0] == dirs[k][0] && D[1] == dirs[k][1] && D[2] == dirs[k][2];
         const bool minus = D[0] == -dirs[k][0] && D[1] == -dirs[k][1] && D[2] == -dirs[k][2];
         if ( !plus && !minus )
            continue;
         F.kind[t] = k + 1;
         for ( int r = 0; r < 3; ++r )
            F.off[t][r] = ( plus ? S[r] : S[r] + D[r] ) - e0[k][r];
      }
      if ( F.kind[t] == 0 )
         return false;
   }
   return true;
}

struct P2FaceSorArgs
{
   double*       u;
   const double* q;
   P2FaceFrame   F[4];
   unsigned      mask;
   int           N, backwards;
   double        relax;
};
__device__ inline int64_t face_edge_index( const P2FaceFrame& F, int n, int t, int i, int j )
{
   const int x = F.O[0] + i * F.a[0] + j * F.b[0] + F.off[t][0], y = F.O[1] + i * F.a[1] + j * F.b[1] + F.off[t][1],
             z = F.O[2] + i * F.a[2] + j * F.b[2] + F.off[t][2];
   return edge_block_start( n, F.kind[t] ) + cell_index( n, x, y, z );
}
// P2::macroface::generated::sor_3D_macroface_P2_update_edgedofs[_backwards] on this cell's copy of the face: rows ascending, x
// ascending, at every index X, XY, Y in place (backwards: everything reversed).  The order only matters between coupled DoFs,
// and the stage 3 ( x + 2 y ) + type puts every DoF after the neighbours the loop visits before it and before the others: one
// workgroup per face walks the stages, all DoFs of a stage at once.
__global__ __launch_bounds__( 256 ) void p2_sor_face_edges_kernel( const P2FaceSorArgs A )
{
   const int f = blockIdx.x;
   if ( !( ( A.mask >> ( 6 + f ) ) & 1u ) )
      return;
   const P2FaceFrame& F = A.F[f];
   const int          n = A.N - 1, stages = 3 * ( 2 * n - 1 );
   for ( int step = 0; step < stages; ++step )
   {
      const int s = A.backwards ? stages - 1 - step : step;
      const int t = s % 3, qq = s / 3;
      const int ylo = qq - n + 1 > 0 ? qq - n + 1 : 0, yhi = qq / 2;
      for ( int y = ylo + (int) threadIdx.x; y <= yhi; y += (int) blockDim.x )
      {
         const int  x     = qq - 2 * y;
         const bool inner = t == 0 ? y >= 1 : ( t == 1 ? x + y <= n - 2 : x >= 1 );
         if ( !inner || x + y > n - 1 )
            continue;
         const int64_t i   = face_edge_index( F, n, t, x, y );
         double        sum = A.q[i];
#pragma unroll
         for ( int k = 0; k < 4; ++k )
            sum -= F.w[t][1 + k] * A.u[face_edge_index( F, n, kFaceNb[t][k][0], x + kFaceNb[t][k][1], y + kFaceNb[t][k][2] )];
         A.u[i] = ( 1.0 - A.relax ) * A.u[i] + A.relax / F.w[t][0] * sum;
      }
      __syncthreads();
   }
}
// the same with the face's edge DoFs staged in LDS in the FACE's layout -- type t, row j, position i at t tri(n) + row_start(n, j) + i --
// (levels <= 6: 3 tri(64) doubles = 50 KB): a stage then costs an LDS round trip and a barrier instead of dependent global loads
// (48 us per call at level 3 with p2_sor_face_edges_kernel, where 45 stages move a few hundred values)
__device__ inline int face_lds_index( int n, int t, int i, int j ) { return t * tri( n ) + row_start( n, j ) + i; }
__device__ inline void p2_sor_face_edges_lds_body( double* u, const double* q, const P2FaceFrame& F, int N, int backwards, double relax )
{
   extern __shared__ double lu[]; // [3][tri(n)]
   const int n = N - 1, T = tri( n ), stages = 3 * ( 2 * n - 1 );
   // every edge DoF of the face plane (inner ones and those on its boundary edges): (t, i, j) with i + j <= n - 1
   for ( int e = threadIdx.x; e < 3 * T; e += (int) blockDim.x )
   {
      const int t = e / T, r = e - t * T;
      const int j = row_of( n, r ), i = r - row_start( n, j );
      lu[e]       = u[face_edge_index( F, n, t, i, j )];
   }
   __syncthreads();
   for ( int step = 0; step < stages; ++step )
   {
      const int s = backwards ? stages - 1 - step : step;
      const int t = s % 3, qq = s / 3;
      const int ylo = qq - n + 1 > 0 ? qq - n + 1 : 0, yhi = qq / 2;
      for ( int y = ylo + (int) threadIdx.x; y <= yhi; y += (int) blockDim.x )
      {
         const int  x     = qq - 2 * y;
         const bool inner = t == 0 ? y >= 1 : ( t == 1 ? x + y <= n - 2 : x >= 1 );
         if ( !inner || x + y > n - 1 )
            continue;
         const int l   = face_lds_index( n, t, x, y );
         double    sum = q[face_edge_index( F, n, t, x, y )];
#pragma unroll
         for ( int k = 0; k < 4; ++k )
            sum -= F.w[t][1 + k] * lu[face_lds_index( n, kFaceNb[t][k][0], x + kFaceNb[t][k][1], y + kFaceNb[t][k][2] )];
         lu[l] = ( 1.0 - relax ) * lu[l] + relax / F.w[t][0] * sum;
      }
      __syncthreads();
   }
   for ( int e = threadIdx.x; e < 3 * T; e += (int) blockDim.x )
   {
      const int  t = e / T, r = e - t * T;
      const int  j = row_of( n, r ), i = r - row_start( n, j );
      const bool inner = t == 0 ? j >= 1 : ( t == 1 ? i + j <= n - 2 : i >= 1 );
      if ( inner )
         u[face_edge_index( F, n, t, i, j )] = lu[e];
   }
}
__global__ __launch_bounds__( 256 ) void p2_sor_face_edges_lds_kernel( const P2FaceSorArgs A )
{
   const int f = blockIdx.x;
   if ( !( ( A.mask >> ( 6 + f ) ) & 1u ) )
      return;
   p2_sor_face_edges_lds_body( A.u, A.q, A.F[f], A.N, A.backwards, A.relax );
}
// up to HYTEG_HIP_MAX_BATCH macro-cells in one launch (blockIdx.y = cell): the cells' face frames (with the faces' total weights) come
// from a device table the caller built once per level (hyteg_hip_p2_sor_face_frames)
struct P2FaceSorBatchArgs
{
   double*            u[HYTEG_HIP_MAX_BATCH];
   const double*      q[HYTEG_HIP_MAX_BATCH];
   unsigned           mask[HYTEG_HIP_MAX_BATCH];
   const P2FaceFrame* frames; // [cell][4]
   int                N, backwards;
   double             relax;
};
__global__ __launch_bounds__( 256 ) void p2_sor_face_edges_lds_batch_kernel( const P2FaceSorBatchArgs A )
{
   const int f = blockIdx.x, cell = blockIdx.y;
   if ( !( ( A.mask[cell] >> ( 6 + f ) ) & 1u ) )
      return;
   __shared__ P2FaceFrame F;
   if ( threadIdx.x == 0 )
      F = A.frames[4 * cell + f];
   __syncthreads();
   p2_sor_face_edges_lds_body( A.u[cell], A.q[cell], F, A.N, A.backwards, A.relax );
}
// the frames F[0..3] of the cell's faces in `mask` (bit 6 + f), origin scaled to the level, with the faces' total weights; the others
// zeroed.  Returns 0, or 1: face_verts[f] are not the three cell-local vertex ids of face f, 2 (only with needDiagonal): a zero
// diagonal weight -- face by face, in that order
int face_frames_of_cell( int level, const int* face_verts, const double* face_w, unsigned mask, bool needDiagonal, P2FaceFrame* F )
{
   const int n = 1 << level;
   for ( int f = 0; f < 4; ++f )
   {
      int cls = 0;
      F[f]    = P2FaceFrame{};
      if ( !( ( mask >> ( 6 + f ) ) & 1u ) )
         continue;
      if ( !face_frame( face_verts + 3 * f, F[f], cls ) || cls != 6 + f )
         return 1;
      for ( int r = 0; r < 3; ++r )
         F[f].O[r] *= n;
      for ( int t = 0; t < 3; ++t )
      {
         if ( needDiagonal && face_w[15 * f + 5 * t] == 0.0 )
            return 2;
         for ( int k = 0; k < 5; ++k )
            F[f].w[t][k] = face_w[15 * f + 5 * t + k];
      }
   }
   return 0;
}
} // namespace
extern "C" {

HYTEG_HIP_API int hyteg_hip_p2_operator_table_face_edge_weights( const double* table_host, const int* face_verts, double* w )
{
   HH_REQUIRE( table_host && face_verts && w, "p2_operator_table_face_edge_weights: null pointer" );
   P2FaceFrame F;
   int         cls = 0;
   HH_REQUIRE( face_frame( face_verts, F, cls ), "p2_operator_table_face_edge_weights: face_verts must be three different cell-local vertex ids" );
   for ( int t = 0; t < 3; ++t )
   {
      const KindStencil S = build_kind_stencil( F.kind[t] );
      for ( int k = 0; k < 5; ++k )
      {
         int kind = F.kind[t], d[3] = { 0, 0, 0 };
         if ( k > 0 )
         {
            const int* nb = kFaceNbHost[t][k - 1];
            kind          = F.kind[nb[0]];
            for ( int r = 0; r < 3; ++r )
               d[r] = nb[1] * F.a[r] + nb[2] * F.b[r] + F.off[nb[0]][r] - F.off[t][r];
         }
         double v = 0.0;
         bool   found = false;
         for ( int q = 0; q < S.n && !found; ++q )
            if ( S.kind[q] == kind && S.dx[q] == d[0] && S.dy[q] == d[1] && S.dz[q] == d[2] )
               v = table_host[class_offset( F.kind[t] ) + ( cls - 0 ) * S.n + q], found = true;
         HH_REQUIRE( found, "p2_operator_table_face_edge_weights: a face neighbour is not in the stencil list (internal error)" );
         w[5 * t + k] = v;
      }
   }
   return HYTEG_HIP_OK;
}

HYTEG_HIP_API int hyteg_hip_p2_sor_face_edgedofs_cell( double* dst_edge, const double* q_edge, int level, const int* face_verts, const double* face_w,
                                                       double relax, unsigned mask, int backwards, hyteg_hip_stream_t stream )
{
   HH_REQUIRE( dst_edge && q_edge && face_verts && face_w, "p2_sor_face_edgedofs_cell: null pointer" );
   HH_REQUIRE( level >= 2 && level <= HYTEG_HIP_P2_MAX_LEVEL, "p2_sor_face_edgedofs_cell: level out of range (2..9)" );
   HH_REQUIRE( dst_edge != q_edge, "p2_sor_face_edgedofs_cell: dst and q must differ" );
   mask &= 0xFu << 6;
   if ( mask == 0 )
      return HYTEG_HIP_OK;
   P2FaceSorArgs A;
   A.u = dst_edge, A.q = q_edge, A.mask = mask, A.N = ( 1 << level ) + 1, A.backwards = backwards ? 1 : 0, A.relax = relax;
   const int n = A.N - 1;
   const int bad = face_frames_of_cell( level, face_verts, face_w, mask, true, A.F );
   HH_REQUIRE( bad != 1, "p2_sor_face_edgedofs_cell: face_verts[f] must be the three cell-local vertex ids of face f" );
   HH_REQUIRE( bad != 2, "p2_sor_face_edgedofs_cell: zero diagonal weight" );
   const size_t lds = (size_t) 3 * tri( n ) * sizeof( double );
   if ( level <= 6 )
   {
      if ( lds > 48 * 1024 )
         HH_CHECK_HIP( hipFuncSetAttribute( reinterpret_cast< const void* >( p2_sor_face_edges_lds_kernel ), hipFuncAttributeMaxDynamicSharedMemorySize,
                                            (int) lds ) );
      hipLaunchKernelGGL( p2_sor_face_edges_lds_kernel, dim3( 4 ), dim3( 256 ), lds, as_stream( stream ), A );
   }
   else
      hipLaunchKernelGGL( p2_sor_face_edges_kernel, dim3( 4 ), dim3( 256 ), 0, as_stream( stream ), A );
   HH_CHECK_HIP( hipGetLastError() );
   return HYTEG_HIP_OK;
}

HYTEG_HIP_API size_t hyteg_hip_p2_sor_face_frames_bytes( void ) { return 4 * sizeof( P2FaceFrame ); }
HYTEG_HIP_API int    hyteg_hip_p2_sor_face_frames( int level, const int* face_verts, const double* face_w, void* frames_host )
{
   HH_REQUIRE( face_verts && face_w && frames_host, "p2_sor_face_frames: null pointer" );
   HH_REQUIRE( level >= 2 && level <= HYTEG_HIP_P2_MAX_LEVEL, "p2_sor_face_frames: level out of range (2..9)" );
   HH_REQUIRE( face_frames_of_cell( level, face_verts, face_w, 0xFu << 6, false, static_cast< P2FaceFrame* >( frames_host ) ) == 0,
               "p2_sor_face_frames: face_verts[f] must be the three cell-local vertex ids of face f" );
   return HYTEG_HIP_OK;
}
HYTEG_HIP_API int hyteg_hip_p2_sor_face_edgedofs_cells( int ncells, double* const* dst_edge, const double* const* q_edge, int level, const void* frames_dev,
                                                        double relax, const unsigned* masks, int backwards, hyteg_hip_stream_t stream )
{
   HH_REQUIRE( dst_edge && q_edge && frames_dev && masks, "p2_sor_face_edgedofs_cells: null pointer" );
   HH_REQUIRE( ncells >= 1 && ncells <= HYTEG_HIP_MAX_BATCH, "p2_sor_face_edgedofs_cells: 1 <= ncells <= HYTEG_HIP_MAX_BATCH" );
   HH_REQUIRE( level >= 2 && level <= 6, "p2_sor_face_edgedofs_cells: levels 2..6 (the face's edge DoFs are staged in LDS)" );
   P2FaceSorBatchArgs A{};
   A.frames = static_cast< const P2FaceFrame* >( frames_dev ), A.N = ( 1 << level ) + 1, A.backwards = backwards ? 1 : 0, A.relax = relax;
   unsigned any = 0;
   for ( int c = 0; c < ncells; ++c )
   {
      HH_REQUIRE( dst_edge[c] && q_edge[c] && dst_edge[c] != q_edge[c], "p2_sor_face_edgedofs_cells: null array, or dst and q are the same" );
      A.u[c] = dst_edge[c], A.q[c] = q_edge[c], A.mask[c] = masks[c] & ( 0xFu << 6 );
      any |= A.mask[c];
   }
   if ( any == 0 )
      return HYTEG_HIP_OK;
   const size_t lds = (size_t) 3 * tri( A.N - 1 ) * sizeof( double );
   if ( lds > 48 * 1024 )
      HH_CHECK_HIP( hipFuncSetAttribute( reinterpret_cast< const void* >( p2_sor_face_edges_lds_batch_kernel ), hipFuncAttributeMaxDynamicSharedMemorySize,
                                         (int) lds ) );
   hipLaunchKernelGGL( p2_sor_face_edges_lds_batch_kernel, dim3( 4, (unsigned) ncells ), dim3( 256 ), lds, as_stream( stream ), A );
   HH_CHECK_HIP( hipGetLastError() );
   return HYTEG_HIP_OK;
}

} // extern "C"
