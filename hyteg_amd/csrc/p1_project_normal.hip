// C-ABI entry points of the strong free-slip condition: the projection ( I - n n^T ) of a velocity onto the tangential
// plane at the boundary points of the macro-cells (P1ProjectNormalOperator, VertexDoFProjectNormal.hpp).  The reference
// evaluates the normal function at every point of every call; here the host layer evaluates it once into a table per
// (cell, level) that is indexed by the shell enumeration of shell.hpp, so that a projection is one launch over the
// shells of all cells of a chunk.  The shell has O(4^L) points: like the kernels of p1_boundary.hip this one is
// latency-bound, which is why every load of a point is issued before its first arithmetic.  The edge-DoF parts of P2 velocities
// are projected by the same body over an enumeration of the shell edge DoFs (EdgeDoFProjectNormal.hpp).
#include "shell.hpp"

using namespace hyteg_hip;

namespace {

constexpr int kThreads = 256;
constexpr int kMaxB    = HYTEG_HIP_MAX_BATCH;

using namespace hyteg_hip::shell;

struct ProjectB
{
   double*       u[kMaxB];
   double*       v[kMaxB];
   double*       w[kMaxB];
   const double* n[kMaxB]; // [3][entries of the enumeration]: component-major, indexed by q
   unsigned      mask[kMaxB];
   int           N; // points per macro-edge (vertex DoFs) or micro-edges per macro-edge (edge DoFs)
};
static_assert( sizeof( ProjectB ) <= 4096, "ProjectB must fit the kernel argument segment" );

// Enumerates every edge DoF on the shell of a macro-cell exactly once: q in [0, 12 tri(n)), n = 2^level micro-edges per macro-edge,
// -> logical index, orientation o (X, Y, Z, XY, XZ, YZ, XYZ = 0..6, edgedofspace/EdgeDoFIndexing.hpp) and macro-primitive slot.
// Per face of the cell the three orientations that lie in it (both end points on the face); an edge DoF on a macro-edge lies in
// two faces and is visited through the lowest-numbered one, the other q returns false.  XYZ edges lie in no face.
__host__ __device__ inline bool shell_edge( int n, int q, int& x, int& y, int& z, int& o, int& slot )
{
   const int T = tri( n );
   if ( q < 0 || q >= 12 * T )
      return false;
   const int ft = q / T, r = q - ft * T;
   const int f = ft / 3, t = ft - 3 * f;
   const int j = row_of( n, r );
   const int i = r - row_start( n, j );
   // orientation t of face f, and the end points relative to the logical index
   const int orient[4][3] = { { 0, 1, 3 }, { 0, 2, 4 }, { 1, 2, 5 }, { 3, 4, 5 } };
   const int ends[6][2][3] = { { { 0, 0, 0 }, { 1, 0, 0 } }, { { 0, 0, 0 }, { 0, 1, 0 } }, { { 0, 0, 0 }, { 0, 0, 1 } },
                               { { 1, 0, 0 }, { 0, 1, 0 } }, { { 1, 0, 0 }, { 0, 0, 1 } }, { { 0, 1, 0 }, { 0, 0, 1 } } };
   o = orient[f][t];
   switch ( f )
   {
   case 0:
      x = i, y = j, z = 0;
      break;
   case 1:
      x = i, y = 0, z = j;
      break;
   case 2:
      x = 0, y = i, z = j;
      break;
   default:
      x = i, y = j, z = n - 1 - i - j;
      break;
   }
   int f0 = 1, f1 = 1, f2 = 1, f3 = 1;
   for ( int e = 0; e < 2; ++e )
   {
      const int px = x + ends[o][e][0], py = y + ends[o][e][1], pz = z + ends[o][e][2];
      f0 &= pz == 0, f1 &= py == 0, f2 &= px == 0, f3 &= px + py + pz == n;
   }
   const int lowest = f0 ? 0 : f1 ? 1 : f2 ? 2 : 3;
   if ( lowest != f )
      return false;
   slot = slot_from_flags< -1 >( f0, f1, f2, f3 );
   return true;
}
// index of edge DoF ( x, y, z, o ), o < 6, in the edge-DoF array of a macro-cell: block o of tet( n ) entries in the cell layout of width n
__host__ __device__ inline int edge_array_index( int n, int x, int y, int z, int o ) { return o * (int) tet32( (unsigned) n ) + cell_index( n, x, y, z ); }

// ( u, v, w ) -= ( ( u, v, w ) . n ) n at array entry i of cell `cell` with the normal of table entry q of S
__device__ inline void project_entry( const ProjectB& A, int cell, int q, int S, int i )
{
   const double* __restrict__ n = A.n[cell];
   double* __restrict__ u = A.u[cell];
   double* __restrict__ v = A.v[cell];
   double* __restrict__ w = A.w[cell];
   const double n0 = n[q], n1 = n[S + q], n2 = n[2 * S + q];
   const double a = u[i], b = v[i], c = w[i];
   const double d = n0 * a + n1 * b + n2 * c;
   u[i]           = a - d * n0;
   v[i]           = b - d * n1;
   w[i]           = c - d * n2;
}

// one thread per q of the shell edge-DoF enumeration, grid.y = cell; A.N holds n = 2^level here
__global__ __launch_bounds__( kThreads ) void p2_edge_project_normal_kernel( const ProjectB A )
{
   const int      q    = blockIdx.x * kThreads + threadIdx.x;
   const int      cell = blockIdx.y;
   const unsigned mask = A.mask[cell];
   int            x, y, z, o, slot;
   if ( !shell_edge( A.N, q, x, y, z, o, slot ) || !( ( mask >> slot ) & 1u ) )
      return;
   project_entry( A, cell, q, 12 * tri( A.N ), edge_array_index( A.N, x, y, z, o ) );
}

// one thread per q of the shell enumeration, grid.y = cell
__global__ __launch_bounds__( kThreads ) void p1_project_normal_kernel( const ProjectB A )
{
   const int      q    = blockIdx.x * kThreads + threadIdx.x;
   const int      cell = blockIdx.y;
   const unsigned mask = A.mask[cell];
   int            x, y, z, slot;
   if ( !shell_point( A.N, q, x, y, z, slot ) || !( ( mask >> slot ) & 1u ) )
      return;
   project_entry( A, cell, q, 4 * tri( A.N ), cell_index( A.N, x, y, z ) );
}

} // namespace

extern "C" {

HYTEG_HIP_API int hyteg_hip_p1_shell_size( int level )
{
   if ( !any_level_ok( level ) )
      return 0;
   return 4 * tri( ( 1 << level ) + 1 );
}

HYTEG_HIP_API int hyteg_hip_p1_shell_enumeration( int level, int* out )
{
   HH_REQUIRE( out, "p1_shell_enumeration: null pointer" );
   HH_REQUIRE( any_level_ok( level ), "p1_shell_enumeration: level out of range [0,11]" );
   const int N = ( 1 << level ) + 1, S = 4 * tri( N );
   for ( int q = 0; q < S; ++q )
   {
      int x = 0, y = 0, z = 0, slot = -1;
      if ( !shell_point( N, q, x, y, z, slot ) )
         slot = -1;
      out[4 * q + 0] = x, out[4 * q + 1] = y, out[4 * q + 2] = z, out[4 * q + 3] = slot;
   }
   return HYTEG_HIP_OK;
}

HYTEG_HIP_API int hyteg_hip_p2_edge_shell_size( int level )
{
   if ( level < 0 || level > HYTEG_HIP_P2_MAX_LEVEL )
      return 0;
   return 12 * tri( 1 << level );
}

HYTEG_HIP_API int hyteg_hip_p2_edge_shell_enumeration( int level, int* out )
{
   HH_REQUIRE( out, "p2_edge_shell_enumeration: null pointer" );
   HH_REQUIRE( level >= 0 && level <= HYTEG_HIP_P2_MAX_LEVEL, "p2_edge_shell_enumeration: level out of range [0,9]" );
   const int n = 1 << level, S = 12 * tri( n );
   for ( int q = 0; q < S; ++q )
   {
      int x = 0, y = 0, z = 0, o = 0, slot = -1;
      if ( !shell_edge( n, q, x, y, z, o, slot ) )
         slot = -1;
      out[5 * q + 0] = x, out[5 * q + 1] = y, out[5 * q + 2] = z, out[5 * q + 3] = o, out[5 * q + 4] = slot;
   }
   return HYTEG_HIP_OK;
}

HYTEG_HIP_API int hyteg_hip_p2_edge_project_normal_cells( int                  ncells,
                                                          double* const*       u,
                                                          double* const*       v,
                                                          double* const*       w,
                                                          const double* const* normals,
                                                          int                  level,
                                                          const unsigned*      masks,
                                                          hyteg_hip_stream_t   stream )
{
   HH_REQUIRE( ncells >= 1 && ncells <= kMaxB, "p2_edge_project_normal_cells: ncells must be 1..HYTEG_HIP_MAX_BATCH" );
   HH_REQUIRE( level >= 0 && level <= HYTEG_HIP_P2_MAX_LEVEL, "p2_edge_project_normal_cells: level out of range [0,9]" );
   HH_REQUIRE( u && v && w && normals && masks, "p2_edge_project_normal_cells: null pointer" );
   ProjectB A{};
   unsigned any = 0;
   for ( int c = 0; c < ncells; ++c )
   {
      HH_REQUIRE( u[c] && v[c] && w[c] && normals[c], "p2_edge_project_normal_cells: null array pointer" );
      HH_REQUIRE( u[c] != v[c] && u[c] != w[c] && v[c] != w[c], "p2_edge_project_normal_cells: the components must not alias" );
      A.u[c] = u[c], A.v[c] = v[c], A.w[c] = w[c], A.n[c] = normals[c];
      A.mask[c] = masks[c] & 0x3FFu; // edge DoFs lie on macro-edges and macro-faces only; inner ones are never projected
      any |= A.mask[c];
   }
   if ( !any )
      return HYTEG_HIP_OK;
   A.N = 1 << level;
   const int blocks = ( 12 * tri( A.N ) + kThreads - 1 ) / kThreads;
   hipLaunchKernelGGL( p2_edge_project_normal_kernel, dim3( blocks, ncells ), dim3( kThreads ), 0, as_stream( stream ), A );
   HH_CHECK_HIP( hipGetLastError() );
   return HYTEG_HIP_OK;
}

HYTEG_HIP_API int hyteg_hip_p1_project_normal_cells( int                  ncells,
                                                     double* const*       u,
                                                     double* const*       v,
                                                     double* const*       w,
                                                     const double* const* normals,
                                                     int                  level,
                                                     const unsigned*      masks,
                                                     hyteg_hip_stream_t   stream )
{
   HH_REQUIRE( ncells >= 1 && ncells <= kMaxB, "p1_project_normal_cells: ncells must be 1..HYTEG_HIP_MAX_BATCH" );
   HH_REQUIRE( any_level_ok( level ), "p1_project_normal_cells: level out of range [0,11]" );
   HH_REQUIRE( u && v && w && normals && masks, "p1_project_normal_cells: null pointer" );
   ProjectB A{};
   unsigned any = 0;
   for ( int c = 0; c < ncells; ++c )
   {
      HH_REQUIRE( u[c] && v[c] && w[c] && normals[c], "p1_project_normal_cells: null array pointer" );
      HH_REQUIRE( u[c] != v[c] && u[c] != w[c] && v[c] != w[c], "p1_project_normal_cells: the components must not alias" );
      A.u[c] = u[c], A.v[c] = v[c], A.w[c] = w[c], A.n[c] = normals[c];
      A.mask[c] = masks[c] & HYTEG_HIP_MASK_SHELL; // inner points are never projected
      any |= A.mask[c];
   }
   if ( !any )
      return HYTEG_HIP_OK;
   A.N = ( 1 << level ) + 1;
   const int blocks = ( 4 * tri( A.N ) + kThreads - 1 ) / kThreads;
   hipLaunchKernelGGL( p1_project_normal_kernel, dim3( blocks, ncells ), dim3( kThreads ), 0, as_stream( stream ), A );
   HH_CHECK_HIP( hipGetLastError() );
   return HYTEG_HIP_OK;
}

} // extern "C"
