// P2 elementwise operator on one macro-cell: dst = alpha * A * src for vertex + edge DoFs, where A is
// given by the 10 x 10 element matrices of the six micro-cell types (constant over an affine macro-cell).
// Reference: P2ElementwiseOperator::gemv / localMatrixVectorMultiply3D (src/hyteg/elementwiseoperators/
// P2ElementwiseOperator.cpp:66-223): a loop over micro-cells that SCATTERS ten sums into the destination arrays.
// Here the operation is a GATHER (no atomics, fixed summation order = the order the reference's scatter loop produces):
// a destination DoF of kind c (vertex, or edge orientation X/Y/Z/XY/XZ/YZ/XYZ) is local DoF k of the micro-cell
// (type t, index dof - offset[t][k]) for a fixed list of (t, k); each such cell contributes row k of its element matrix
// times its ten source values.  The lists and offsets follow from celldof::macrocell::getMicroVerticesFromMicroCell
// (volumedofspace/CellDoFIndexing.hpp:155-198) and edgedof::calcEdgeDoFIndex / calcEdgeDoFOrientation
// (edgedofspace/EdgeDoFIndexing.hpp:89-165); they are built once on the host.
// Kernels, by level: levels 0-1 the table-driven micro-cell gather (p2_elementwise_kernel, one thread group per DoF);
// level 2 and kind-restricted applies below level 6: compile-time stencils, thread per DoF (p2_inner_body, p2_boundary_body) or by
// rows (p2_rows_body_dpp); from level 3: p2_class_rows_kernel -- row waves that compute the inner DoFs and every boundary class
// (round 3, kernels_p2_class_rows.hpp).
// This file: the operator-table builders and the two apply entry points (one macro-cell, a batch); the kernels are in
// kernels_p2_gather.hpp, kernels_p2_threads.hpp, kernels_p2_rows.hpp and kernels_p2_class_rows.hpp.  The edge-DoF vector
// operations are in p2_edge_vector.hip, the constant-stencil seam in p2_constant_seam.hip, the macro-face SOR in p2_sor_face.hip.
#include <algorithm>
#include <atomic>
#include <mutex>
#include <utility>
#include <vector>

#include "device_table.hpp"
#include "kernels_p2_class_rows.hpp"
#include "kernels_p2_gather.hpp"

namespace {

// first level the row kernel with every point class is used at (HYTEG_HIP_P2_CLASS_ROWS_MIN_LEVEL, hyteg_hip_p2_set_class_rows_min_level: tests run it at small
// levels, 99 = the row kernel of round 2 at every level)
std::atomic< int >& class_rows_min_level()
{
   static std::atomic< int > v( env_int( "HYTEG_HIP_P2_CLASS_ROWS_MIN_LEVEL", kClassRowsMinLevel ) );
   return v;
}

// tiles of the row kernel with every point class: (x0, y, z) with x0 a multiple of the capacity (62 positions per lane position), over the positions (x, y, z) with x + y + z <= N - 2 (where some kind
// has a DoF off the planes x = 0 and x + y + z = n)
int get_class_rows_tiles( int level, int capacity, TileTable* out )
{
   static DeviceTableCache< std::pair< int, int >, TileTable > cache;
   const TileTable*                                             tt = nullptr;
   const int rc = cache.get( std::make_pair( level, capacity ),
                             [&]( TileTable& t ) {
                                const int           N = ( 1 << level ) + 1;
                                std::vector< Tile > host;
                                for ( int z = 0; z <= N - 1; ++z )
                                   for ( int y = 0; y <= N - 1 - z; ++y )
                                      for ( int x0 = 0; x0 <= N - 1 - y - z; x0 += capacity )
                                      {
                                         Tile tl{};
                                         tl.a      = cell_index( N, x0, y, z );
                                         tl.pad[0] = cell_index( N - 1, x0, y, z );
                                         tl.pad[1] = cell_index( N - 2, x0, y, z );
                                         tl.ya = y, tl.yb = x0, tl.z = z;
                                         tl.cnt = std::min( capacity, N - y - z - x0 );
                                         host.push_back( tl );
                                      }
                                t.count = (int) host.size();
                                return upload_table( host, &t.dev );
                             },
                             &tt );
   if ( rc == HYTEG_HIP_OK )
      *out = *tt;
   return rc;
}

// host: does micro-cell (type t, index m) lie inside a macro-cell of width N?
bool micro_cell_inside( int t, int mx, int my, int mz, int N )
{
   for ( int v = 0; v < 4; ++v )
   {
      const int x = mx + cMicroVerts[t][v][0], y = my + cMicroVerts[t][v][1], z = mz + cMicroVerts[t][v][2];
      if ( x < 0 || y < 0 || z < 0 || x + y + z > N - 1 )
         return false;
   }
   return true;
}
int host_class_of( int c, int x, int y, int z, int N )
{
   int       f[4] = { 1, 1, 1, 1 };
   const int npts = c == 0 ? 1 : 2;
   for ( int e = 0; e < npts; ++e )
   {
      const int px = x + ( c == 0 ? 0 : kEdgeEndsHost[c - 1][e][0] ), py = y + ( c == 0 ? 0 : kEdgeEndsHost[c - 1][e][1] ),
                pz = z + ( c == 0 ? 0 : kEdgeEndsHost[c - 1][e][2] );
      f[0] &= pz == 0, f[1] &= py == 0, f[2] &= px == 0, f[3] &= px + py + pz == N - 1;
   }
   return slot_from_flags< 14 >( f[0], f[1], f[2], f[3] );
}

// faces of the cell (bit g; 0: z = 0, 1: y = 0, 2: x = 0, 3: x + y + z = n) that contain the macro-primitive of point class cls
int class_face_flags( int cls )
{
   static const int edges[6] = { 0x3, 0x5, 0x9, 0x6, 0xA, 0xC }, verts[4] = { 0x7, 0xB, 0xD, 0xE };
   return cls < 6 ? edges[cls] : ( cls < 10 ? 1 << ( cls - 6 ) : verts[cls - 10] );
}
int plane_fn( int g, const int* p ) { return g == 0 ? p[2] : ( g == 1 ? p[1] : ( g == 2 ? p[0] : -( p[0] + p[1] + p[2] ) ) ); }
// the micro-vertices a DoF of a kind sits on, relative to its logical index (vertex DoF: one; edge DoF: its two end points)
int kind_points( int kind, int pts[2][3] )
{
   if ( kind == 0 )
   {
      pts[0][0] = pts[0][1] = pts[0][2] = 0;
      return 1;
   }
   for ( int e = 0; e < 2; ++e )
      for ( int r = 0; r < 3; ++r )
         pts[e][r] = kEdgeEndsHost[kind - 1][e][r];
   return 2;
}
// does the source DoF (kind K at offset d from a destination DoF of kind C and point class cls) lie on the closure of the
// destination's macro-primitive, i.e. on every cell face that contains it?  A question about offsets only.
bool source_on_closure( int C, int cls, int K, int dx, int dy, int dz )
{
   int       pd[2][3], ps[2][3];
   const int nd = kind_points( C, pd ), ns = kind_points( K, ps ), flags = class_face_flags( cls );
   for ( int g = 0; g < 4; ++g )
   {
      if ( !( ( flags >> g ) & 1 ) )
         continue;
      const int h = plane_fn( g, pd[0] );
      for ( int e = 1; e < nd; ++e )
         if ( plane_fn( g, pd[e] ) != h )
            return false; // a DoF of this kind cannot lie on that face at all: the class row is never used
      for ( int e = 0; e < ns; ++e )
      {
         const int q[3] = { dx + ps[e][0], dy + ps[e][1], dz + ps[e][2] };
         if ( plane_fn( g, q ) != h )
            return false;
      }
   }
   return true;
}

// ---- what the two apply entry points share ----
// this call takes the row kernel with every point class.  A kind-restricted apply (the per-type sweeps of the Gauss-Seidel smoother)
// takes it from level 6: below, where the launches are latency-bound, the kernels of round 2 were 5 % faster on the sweep
// (profiles/r03_p2_class_rows.txt (D))
bool takes_class_rows( int level, unsigned kind_mask )
{
   return level >= class_rows_min_level().load( std::memory_order_relaxed ) && ( kind_mask == 0xFFu || level >= 6 );
}
// arguments of a row kernel over the tile table tt with `waves` tiles per workgroup; *blocks = its grid.  With xcdChunks, a grid of 64
// blocks or more is rounded up to eight equal chunks, one per XCD (p2_rows_body)
P2RowsArgs rows_args( const P2FastArgs& F, const TileTable& tt, int waves, bool xcdChunks, unsigned* blocks )
{
   P2RowsArgs R;
   R.F = F, R.tiles = tt.dev, R.ntiles = tt.count, R.xcd_chunk = 0;
   const int n = F.N - 1;
   R.vbytes    = (unsigned) ( tet64( F.N ) * 8 );
   R.ebytes    = (unsigned) ( ( 6 * tet64( n ) + tet64( n - 1 ) ) * 8 );
   *blocks     = (unsigned) ( ( tt.count + waves - 1 ) / waves );
   if ( xcdChunks && *blocks >= 64 )
   {
      R.xcd_chunk = (int) ( ( *blocks + 7 ) / 8 );
      *blocks     = 8u * (unsigned) R.xcd_chunk;
   }
   return R;
}
// launch( UPDATE, RESTRICTED ) with the two as compile-time constants (std::integral_constant), chosen from the call's update type
// and from whether it computes some destination kinds only
template < typename Launch >
void with_update_and_restriction( int update, bool restricted, Launch&& launch )
{
   using Add     = std::integral_constant< int, HYTEG_HIP_ADD >;
   using Replace = std::integral_constant< int, HYTEG_HIP_REPLACE >;
   if ( restricted && update == HYTEG_HIP_ADD )
      launch( Add{}, std::true_type{} );
   else if ( restricted )
      launch( Replace{}, std::true_type{} );
   else if ( update == HYTEG_HIP_ADD )
      launch( Add{}, std::false_type{} );
   else
      launch( Replace{}, std::false_type{} );
}

} // namespace

extern "C" {

HYTEG_HIP_API size_t hyteg_hip_p2_operator_table_size( void ) { return (size_t) kOperatorTableSize; }

HYTEG_HIP_API int hyteg_hip_p2_set_class_rows_min_level( int level )
{
   const int before = class_rows_min_level().load();
   class_rows_min_level().store( level < 3 ? 3 : level );
   return before;
}

HYTEG_HIP_API int hyteg_hip_p2_build_operator_table( const double* elmat_host, double* table_host )
{
   HH_REQUIRE( elmat_host && table_host, "p2_build_operator_table: null pointer" );
   for ( int k = 0; k < 600; ++k )
      table_host[k] = elmat_host[k];
   for ( int c = 0; c < 8; ++c )
   {
      const KindStencil S   = build_kind_stencil( c );
      double*           w   = table_host + stencil_offset( c );
      for ( int q = 0; q < S.n; ++q )
         w[q] = 0.0;
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
               for ( int q = 0; q < S.n; ++q )
                  if ( S.kind[q] == col.kind && S.dx[q] == dx && S.dy[q] == dy && S.dz[q] == dz )
                     w[q] += elmat_host[100 * t + 10 * k + j];
            }
         }
      // boundary classes: the adjacent micro-cells that exist are read off a representative DoF of that class at level 3
      const int Nr = 9, nr = 8, Wr = c == 0 ? Nr : ( c == 7 ? nr - 1 : nr );
      double*   wc = table_host + class_offset( c );
      for ( int k = 0; k < 14 * S.n; ++k )
         wc[k] = 0.0;
      for ( int cls = 0; cls < 14; ++cls )
      {
         bool found = false;
         for ( int z = 0; z < Wr && !found; ++z )
            for ( int y = 0; y < Wr - z && !found; ++y )
               for ( int x = 0; x < Wr - z - y && !found; ++x )
               {
                  if ( host_class_of( c, x, y, z, Nr ) != cls )
                     continue;
                  found = true;
                  for ( int t = 0; t < 6; ++t )
                     for ( int k = 0; k < 10; ++k )
                     {
                        const CLocal row = c_local( t, k );
                        if ( row.kind != c || !micro_cell_inside( t, x - row.ox, y - row.oy, z - row.oz, Nr ) )
                           continue;
                        for ( int j = 0; j < 10; ++j )
                        {
                           const CLocal col = c_local( t, j );
                           const int    dx = col.ox - row.ox, dy = col.oy - row.oy, dz = col.oz - row.oz;
                           for ( int q = 0; q < S.n; ++q )
                              if ( S.kind[q] == col.kind && S.dx[q] == dx && S.dy[q] == dy && S.dz[q] == dz )
                                 wc[cls * S.n + q] += elmat_host[100 * t + 10 * k + j];
                        }
                     }
               }
      }
   }
   return HYTEG_HIP_OK;
}

HYTEG_HIP_API int hyteg_hip_p2_elementwise_apply_cell( double*            dst_vertex,
                                                       double*            dst_edge,
                                                       const double*      src_vertex,
                                                       const double*      src_edge,
                                                       int                level,
                                                       const double*      optable_dev,
                                                       double             alpha,
                                                       int                update,
                                                       unsigned           mask,
                                                       hyteg_hip_stream_t stream )
{
   return hyteg_hip_p2_elementwise_apply_cell_kinds( dst_vertex, dst_edge, src_vertex, src_edge, level, optable_dev, alpha, update, mask, 0xFFu,
                                                     stream );
}

HYTEG_HIP_API int hyteg_hip_p2_elementwise_apply_cell_kinds( double*            dst_vertex,
                                                             double*            dst_edge,
                                                             const double*      src_vertex,
                                                             const double*      src_edge,
                                                             int                level,
                                                             const double*      optable_dev,
                                                             double             alpha,
                                                             int                update,
                                                             unsigned           mask,
                                                             unsigned           kind_mask,
                                                             hyteg_hip_stream_t stream )
{
   HH_REQUIRE( dst_vertex && dst_edge && src_vertex && src_edge && optable_dev, "p2_elementwise_apply_cell: null pointer" );
   HH_REQUIRE( level >= 0 && level <= HYTEG_HIP_P2_MAX_LEVEL, "p2_elementwise_apply_cell: level out of range [0,9]" );
   HH_REQUIRE( dst_vertex != src_vertex && dst_edge != src_edge, "p2_elementwise_apply_cell: src and dst must not alias" );
   HH_REQUIRE( update == HYTEG_HIP_REPLACE || update == HYTEG_HIP_ADD, "p2_elementwise_apply_cell: bad update type" );
   mask &= HYTEG_HIP_MASK_ALL;
   kind_mask &= 0xFFu;
   if ( mask == 0 || kind_mask == 0 )
      return HYTEG_HIP_OK;
   hipStream_t       s = as_stream( stream );
   static const bool perThread = env_flag( "HYTEG_HIP_P2_INNER_THREADS", false ); // measurement switch: round 1's thread-per-DoF kernel, two launches
   P2FastArgs F;
   F.dstV = dst_vertex, F.dstE = dst_edge, F.srcV = src_vertex, F.srcE = src_edge, F.table = optable_dev, F.alpha = alpha;
   F.N = ( 1 << level ) + 1, F.update = update, F.kinds = kind_mask;
   const int  faces = 4 * tri( F.N );
   const int  nbx   = ( faces + kThreads - 1 ) / kThreads;
   const bool rows  = ( mask & HYTEG_HIP_MASK_INNER ) && level >= 3 && !perThread;
   const bool restricted = kind_mask != 0xFFu;
   if ( level >= 3 && !perThread && takes_class_rows( level, kind_mask ) )
   {
      // one launch of row waves for the inner DoFs and every boundary class (all kinds, or the kinds of kind_mask)
      TileTable tt;
      const int rc = get_class_rows_tiles( level, 62, &tt );
      if ( rc != HYTEG_HIP_OK )
         return rc;
      unsigned         waveBlocks;
      const P2RowsArgs R = rows_args( F, tt, kClassRowsWaves, true, &waveBlocks );
      with_update_and_restriction( update, restricted, [&]( auto upd, auto res ) {
         hipLaunchKernelGGL( ( p2_class_rows_kernel< upd(), 1, res() > ), dim3( waveBlocks ), dim3( 64 * kClassRowsWaves ), 0, s, R.tiles, R.ntiles, R.xcd_chunk, R,
                             mask );
      } );
      HH_CHECK_HIP( hipGetLastError() );
      return HYTEG_HIP_OK;
   }
   if ( rows )
   {
      // inner DoFs by rows (p2_rows_body_dpp: every source row loaded once, 62 positions per wave; HYTEG_HIP_P2_ROWS_DPP=0 selects
      // p2_rows_body: every source loaded, 64 positions); the boundary DoFs, if asked for, in the same launch
      static const bool dpp = env_flag( "HYTEG_HIP_P2_ROWS_DPP", true );
      TileTable tt;
      const int rc = get_tiles( level, TILES_ROWS, dpp ? kRowsDppCapacity : 64, &tt );
      if ( rc != HYTEG_HIP_OK )
         return rc;
      static const bool xcdRows = env_flag( "HYTEG_HIP_P2_XCD_ROWS", true );
      unsigned          rowBlocks;
      const P2RowsArgs  R     = rows_args( F, tt, kRowsWaves, xcdRows, &rowBlocks );
      const unsigned    shell = mask & HYTEG_HIP_MASK_SHELL;
      const int         nb    = shell ? nbx : 0;
      const dim3        block( kThreads );
      // some kinds only: the boundary DoFs (their kernel skips the other kinds) in their own launch, the rows restricted
      if ( restricted && nb )
      {
         P2ClassArgs B;
         B.F = F, B.mask = shell;
         hipLaunchKernelGGL( p2_boundary_kernel, dim3( (unsigned) nbx, 8 ), dim3( kThreads ), 0, s, B );
      }
      with_update_and_restriction( update, restricted, [&]( auto upd, auto res ) {
         if constexpr ( !res() )
            if ( nb != 0 )
            {
               if ( dpp )
                  hipLaunchKernelGGL( ( p2_apply_fused_kernel< upd(), true > ), dim3( 8 * nb + rowBlocks ), block, 0, s, R.tiles, R.ntiles, R.xcd_chunk, R, shell,
                                      nb );
               else
                  hipLaunchKernelGGL( ( p2_apply_fused_kernel< upd(), false > ), dim3( 8 * nb + rowBlocks ), block, 0, s, R.tiles, R.ntiles, R.xcd_chunk, R, shell,
                                      nb );
               return;
            }
         if ( dpp )
            hipLaunchKernelGGL( ( p2_rows_kernel< upd(), res(), true > ), dim3( rowBlocks ), block, 0, s, R.tiles, R.ntiles, R.xcd_chunk, R );
         else
            hipLaunchKernelGGL( ( p2_rows_kernel< upd(), res(), false > ), dim3( rowBlocks ), block, 0, s, R.tiles, R.ntiles, R.xcd_chunk, R );
      } );
      HH_CHECK_HIP( hipGetLastError() );
      return HYTEG_HIP_OK;
   }
   if ( mask & HYTEG_HIP_MASK_INNER )
   {
      // inner DoFs: compile-time stencils, one thread per DoF, all destination kinds in one launch
      const int64_t largest = tet64( F.N );
      hipLaunchKernelGGL( p2_inner_kernel, dim3( (unsigned) ( ( largest + kThreads - 1 ) / kThreads ), 8 ), dim3( kThreads ), 0, s, F );
   }
   if ( ( mask & HYTEG_HIP_MASK_SHELL ) && level >= 2 )
   {
      // DoFs on the macro-cell boundary: per-class constant stencils
      P2ClassArgs B;
      B.F = F, B.mask = mask & HYTEG_HIP_MASK_SHELL;
      hipLaunchKernelGGL( p2_boundary_kernel, dim3( (unsigned) nbx, 8 ), dim3( kThreads ), 0, s, B );
   }
   else if ( mask & HYTEG_HIP_MASK_SHELL )
   {
      // levels 0 and 1: a DoF can be next to several macro-faces at once; micro-cell by micro-cell gather in the reference's order
      P2Args A;
      A.dstV = dst_vertex, A.dstE = dst_edge, A.srcV = src_vertex, A.srcE = src_edge, A.elmat = optable_dev, A.alpha = alpha;
      A.N = ( 1 << level ) + 1, A.update = update, A.mask = mask & HYTEG_HIP_MASK_SHELL, A.kinds = kind_mask, A.T = tables();
      const int     faces = 4 * tri( A.N ); // candidates of the widest kind
      constexpr int G     = 8;
      hipLaunchKernelGGL( p2_elementwise_kernel< G >, dim3( (unsigned) ( ( faces + kThreads / G - 1 ) / ( kThreads / G ) ), 8 ), dim3( kThreads ), 0,
                          s, A );
   }
   HH_CHECK_HIP( hipGetLastError() );
   return HYTEG_HIP_OK;
}

HYTEG_HIP_API int hyteg_hip_p2_elementwise_apply_cells_kinds( int ncells, double* const* dst_vertex, double* const* dst_edge, const double* const* src_vertex,
                                                              const double* const* src_edge, int level, const double* const* optables_dev, double alpha,
                                                              int update, const unsigned* masks, unsigned kind_mask, hyteg_hip_stream_t stream )
{
   HH_REQUIRE( dst_vertex && dst_edge && src_vertex && src_edge && optables_dev && masks, "p2_elementwise_apply_cells_kinds: null pointer" );
   HH_REQUIRE( ncells >= 1 && ncells <= HYTEG_HIP_MAX_BATCH, "p2_elementwise_apply_cells_kinds: 1 <= ncells <= HYTEG_HIP_MAX_BATCH" );
   HH_REQUIRE( level >= 2 && level <= 6, "p2_elementwise_apply_cells_kinds: levels 2..6 (below: the micro-cell gather per cell; above: the row kernels per cell)" );
   HH_REQUIRE( update == HYTEG_HIP_REPLACE || update == HYTEG_HIP_ADD, "p2_elementwise_apply_cells_kinds: bad update" );
   kind_mask &= 0xFFu;
   if ( kind_mask == 0 )
      return HYTEG_HIP_OK;
   P2BatchPtrs P{};
   unsigned    any = 0;
   for ( int c = 0; c < ncells; ++c )
   {
      HH_REQUIRE( dst_vertex[c] && dst_edge[c] && src_vertex[c] && src_edge[c] && optables_dev[c], "p2_elementwise_apply_cells_kinds: null array" );
      HH_REQUIRE( dst_vertex[c] != src_vertex[c] && dst_edge[c] != src_edge[c], "p2_elementwise_apply_cells_kinds: dst and src must differ" );
      P.dstV[c] = dst_vertex[c], P.dstE[c] = dst_edge[c], P.srcV[c] = src_vertex[c], P.srcE[c] = src_edge[c], P.table[c] = optables_dev[c];
      P.mask[c] = masks[c] & HYTEG_HIP_MASK_ALL;
      any |= P.mask[c];
   }
   if ( any == 0 )
      return HYTEG_HIP_OK;
   P2FastArgs F{};
   F.alpha = alpha, F.N = ( 1 << level ) + 1, F.update = update, F.kinds = kind_mask;
   hipStream_t s = as_stream( stream );
   if ( takes_class_rows( level, kind_mask ) )
   {
      // row waves for the inner DoFs and every boundary class of every cell, one launch (all kinds; a kind mask from level 6)
      TileTable tt;
      const int rc = get_class_rows_tiles( level, 62, &tt );
      if ( rc != HYTEG_HIP_OK )
         return rc;
      unsigned         waveBlocks;
      const P2RowsArgs R = rows_args( F, tt, kClassRowsWaves, false, &waveBlocks );
      const dim3       grid( waveBlocks, (unsigned) ncells );
      with_update_and_restriction( update, kind_mask != 0xFFu, [&]( auto upd, auto res ) {
         hipLaunchKernelGGL( ( p2_class_rows_batch_kernel< upd(), res() > ), grid, dim3( 64 * kClassRowsWaves ), 0, s, R.tiles, R.ntiles, R, P );
      } );
      HH_CHECK_HIP( hipGetLastError() );
      return HYTEG_HIP_OK;
   }
   if ( any & HYTEG_HIP_MASK_INNER )
   {
      const int64_t largest = tet64( F.N );
      hipLaunchKernelGGL( p2_inner_batch_kernel, dim3( (unsigned) ( ( largest + kThreads - 1 ) / kThreads ), 8, (unsigned) ncells ), dim3( kThreads ), 0, s, F, P );
   }
   if ( any & HYTEG_HIP_MASK_SHELL )
   {
      const int nbx = ( 4 * tri( F.N ) + kThreads - 1 ) / kThreads;
      hipLaunchKernelGGL( p2_boundary_batch_kernel, dim3( (unsigned) nbx, 8, (unsigned) ncells ), dim3( kThreads ), 0, s, F, P );
   }
   HH_CHECK_HIP( hipGetLastError() );
   return HYTEG_HIP_OK;
}

HYTEG_HIP_API int hyteg_hip_p2_operator_table_closure_split( const double* table_host, double* outside, double* closure_vertex, double* closure_edge )
{
   HH_REQUIRE( table_host && outside && closure_vertex && closure_edge, "p2_operator_table_closure_split: null pointer" );
   for ( int k = 0; k < kOperatorTableSize; ++k )
      outside[k] = closure_vertex[k] = closure_edge[k] = 0.0;
   for ( int c = 0; c < 8; ++c )
   {
      const KindStencil S = build_kind_stencil( c );
      for ( int cls = 0; cls < 14; ++cls )
         for ( int q = 0; q < S.n; ++q )
         {
            const int    at = class_offset( c ) + cls * S.n + q;
            const double w  = table_host[at];
            if ( source_on_closure( c, cls, S.kind[q], S.dx[q], S.dy[q], S.dz[q] ) )
               ( S.kind[q] == 0 ? closure_vertex : closure_edge )[at] = w;
            else
               outside[at] = w;
         }
   }
   return HYTEG_HIP_OK;
}

} // extern "C"
