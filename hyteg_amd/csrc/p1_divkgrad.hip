// C-ABI entry points of the variable-coefficient P1 diffusion operator -div( k grad u ) on one macro-cell: the seam of the generated
// operatorgeneration::P1ElementwiseDivKGrad (apply_macro_3D / computeInverseDiagonalOperatorValues_macro_3D of module
// hyteg_operators; known-answer test tests/hyteg/convergence/ElementwiseDivKGradCGConvergenceTest.cpp) and the fused form of
// P1ElementwiseOperator::smooth_jac (src/hyteg/elementwiseoperators/P1ElementwiseOperator.cpp:288-331).  Kernels: kernels_divkgrad.hpp.
#include <cmath>

#include "kernels_divkgrad.hpp"

using namespace hyteg_hip;
using namespace hyteg_hip::divkgrad;

namespace {

constexpr int kMaxLevel = 8;

// Brick shape of the z-march: rows x slices per wave (loads run one slice ahead).  The kernel holds two arrays in registers, so its
// bricks are lower than the constant-stencil kernel's.  Levels <= 7 are a few hundred bricks: many short waves; level 8 marches
// eight slices so that fewer slices are loaded twice.  hyteg_hip_p1_elementwise_divkgrad_set_shape overrides (tests, measurements).
struct Shape
{
   int ny, lz;
};
Shape g_shape_override{ 0, 0 };
#define HYTEG_DKG_SHAPES( X ) X( 2, 4 ) X( 2, 8 ) X( 1, 8 )
inline Shape shape_of( int level )
{
   if ( g_shape_override.ny )
      return g_shape_override;
   return level <= 7 ? Shape{ 2, 4 } : Shape{ 2, 8 };
}
inline bool shape_compiled( const Shape& s )
{
#define HH_X( NY_, LZ_ ) \
   if ( s.ny == NY_ && s.lz == LZ_ ) \
      return true;
   HYTEG_DKG_SHAPES( HH_X )
#undef HH_X
   return false;
}

int level_of( int64_t micro_edges, int* level )
{
   if ( micro_edges < 1 || ( micro_edges & ( micro_edges - 1 ) ) != 0 )
      return HYTEG_HIP_EINVAL;
   int l = 0;
   while ( ( (int64_t) 1 << l ) < micro_edges )
      ++l;
   *level = l;
   return HYTEG_HIP_OK;
}

// validation of what every entry shares, and the weights: 0.25 K_t of the six micro-cell types
int prepare( const char* who, const double* coords, int64_t micro_edges, Args& A, int* level )
{
   const std::string w( who );
   HH_REQUIRE( coords, w + ": null pointer" );
   HH_REQUIRE( level_of( micro_edges, level ) == HYTEG_HIP_OK && *level <= kMaxLevel,
               w + ": micro_edges_per_macro_edge must be a power of two, at most 2^8" );
   double cc[4][3];
   for ( int v = 0; v < 4; ++v )
      for ( int r = 0; r < 3; ++r )
         cc[v][r] = coords[3 * v + r];
   double       g[4][3];
   const double V = elmat::gradients( cc, g );
   HH_REQUIRE( V > 0.0 && std::isfinite( V ), w + ": degenerate macro-cell" );
   for ( int t = 0; t < 6; ++t )
   {
      double c[4][3], Ke[4][4];
      elmat::micro_cell_coords( cc, micro_edges, t, c );
      elmat::p1_diffusion( c, Ke );
      for ( int a = 0; a < 4; ++a )
      {
         A.W.diag[t][a] = 0.25 * Ke[a][a];
         for ( int b = a + 1; b < 4; ++b )
            A.W.off[t][pair_index( a, b )] = 0.25 * Ke[a][b];
      }
   }
   A.N     = ( 1 << *level ) + 1;
   A.bytes = (unsigned) ( tet64( A.N ) * (int64_t) sizeof( double ) );
   return HYTEG_HIP_OK;
}

inline int shell_blocks( int N ) { return ( 4 * tri( N ) + kPointThreads - 1 ) / kPointThreads; }

template < int MODE >
int launch_shell( const Args& A, unsigned mask, hipStream_t stream )
{
   hipLaunchKernelGGL( divkgrad_shell_kernel< MODE >, dim3( shell_blocks( A.N ) ), dim3( kPointThreads ), 0, stream, A, mask );
   HH_CHECK_HIP( hipGetLastError() );
   return HYTEG_HIP_OK;
}

template < int MODE >
int launch_inner_points( const Args& A, int level, hipStream_t stream )
{
   TileTable tt;
   const int rc = get_tiles( level, TILES_FULL, 1024, &tt );
   if ( rc != HYTEG_HIP_OK || tt.count == 0 )
      return rc;
   hipLaunchKernelGGL( divkgrad_inner_point_kernel< MODE >, dim3( tt.count ), dim3( kPointThreads ), 0, stream, A, tt.dev, tt.count );
   HH_CHECK_HIP( hipGetLastError() );
   return HYTEG_HIP_OK;
}

// measurement switch (tools/bench_kernels.py): the inner points by the one-thread-per-point kernel instead of the z-march
bool g_inner_by_points = false;

template < int MODE >
int launch_inner( const Args& A, int level, hipStream_t stream )
{
   if ( level < HYTEG_HIP_MIN_LEVEL )
      return HYTEG_HIP_OK; // no inner points
   if ( g_inner_by_points )
      return launch_inner_points< MODE >( A, level, stream );
   const Shape s = shape_of( level );
   BrickTable  bt;
   const int   rc = get_bricks( level, s.ny, s.lz, &bt );
   if ( rc != HYTEG_HIP_OK || bt.count == 0 )
      return rc;
   int nblocks          = ( bt.count + kZMarchWavesPerBlock - 1 ) / kZMarchWavesPerBlock;
   nblocks              = ( nblocks + 7 ) & ~7;
   const int xcd_chunk  = nblocks / 8; // consecutive bricks on one XCD, as in the constant-stencil apply
#define HH_X( NY_, LZ_ )                                                                                                                         \
   if ( s.ny == NY_ && s.lz == LZ_ )                                                                                                             \
      hipLaunchKernelGGL( ( divkgrad_zmarch_kernel< MODE, NY_, LZ_, 1 > ), dim3( nblocks ), dim3( 64 * kZMarchWavesPerBlock ), 0, stream, bt.dev, \
                          bt.count, xcd_chunk, A );
   HYTEG_DKG_SHAPES( HH_X )
#undef HH_X
   HH_CHECK_HIP( hipGetLastError() );
   return HYTEG_HIP_OK;
}

} // namespace

extern "C" {

HYTEG_HIP_API int hyteg_hip_p1_elementwise_divkgrad_apply_macro_3d_masked( double*            dst,
                                                                           const double*      src,
                                                                           const double*      k,
                                                                           const double*      macro_vertex_coords,
                                                                           int64_t            micro_edges_per_macro_edge,
                                                                           unsigned           mask,
                                                                           int                update,
                                                                           hyteg_hip_stream_t stream )
{
   const char* who = "p1_elementwise_divkgrad_apply_macro_3d";
   HH_REQUIRE( dst && src && k && macro_vertex_coords, std::string( who ) + ": null pointer" );
   HH_REQUIRE( dst != src && dst != k, std::string( who ) + ": dst must not alias src or k" );
   HH_REQUIRE( update == HYTEG_HIP_REPLACE || update == HYTEG_HIP_ADD, std::string( who ) + ": bad update type" );
   HH_REQUIRE( ( mask & ~(unsigned) HYTEG_HIP_MASK_ALL ) == 0, std::string( who ) + ": bad mask (15 class bits)" );
   Args A{};
   int  level = 0;
   int  rc    = prepare( who, macro_vertex_coords, micro_edges_per_macro_edge, A, &level );
   if ( rc != HYTEG_HIP_OK )
      return rc;
   A.dst = dst, A.src = src, A.k = k;
   const bool add = update == HYTEG_HIP_ADD;
   if ( mask & HYTEG_HIP_MASK_SHELL )
   {
      rc = add ? launch_shell< DKG_ADD >( A, mask & HYTEG_HIP_MASK_SHELL, as_stream( stream ) ) :
                 launch_shell< DKG_REPLACE >( A, mask & HYTEG_HIP_MASK_SHELL, as_stream( stream ) );
      if ( rc != HYTEG_HIP_OK )
         return rc;
   }
   if ( mask & HYTEG_HIP_MASK_INNER )
      return add ? launch_inner< DKG_ADD >( A, level, as_stream( stream ) ) : launch_inner< DKG_REPLACE >( A, level, as_stream( stream ) );
   return HYTEG_HIP_OK;
}

HYTEG_HIP_API int hyteg_hip_p1_elementwise_divkgrad_jacobi_macro_3d( double*            dst,
                                                                     const double*      src,
                                                                     const double*      rhs,
                                                                     const double*      inv_diag,
                                                                     const double*      k,
                                                                     const double*      macro_vertex_coords,
                                                                     int64_t            micro_edges_per_macro_edge,
                                                                     double             omega,
                                                                     hyteg_hip_stream_t stream )
{
   const char* who = "p1_elementwise_divkgrad_jacobi_macro_3d";
   HH_REQUIRE( dst && src && rhs && inv_diag && k && macro_vertex_coords, std::string( who ) + ": null pointer" );
   HH_REQUIRE( dst != src && dst != k && dst != rhs && dst != inv_diag, std::string( who ) + ": dst must not alias an input" );
   Args A{};
   int  level = 0;
   int  rc    = prepare( who, macro_vertex_coords, micro_edges_per_macro_edge, A, &level );
   if ( rc != HYTEG_HIP_OK )
      return rc;
   A.dst = dst, A.src = src, A.k = k, A.rhs = rhs, A.invdiag = inv_diag, A.omega = omega;
   return launch_inner< DKG_JACOBI >( A, level, as_stream( stream ) );
}

HYTEG_HIP_API int hyteg_hip_p1_elementwise_divkgrad_diagonal_macro_3d( double*            diag,
                                                                       const double*      k,
                                                                       const double*      macro_vertex_coords,
                                                                       int64_t            micro_edges_per_macro_edge,
                                                                       hyteg_hip_stream_t stream )
{
   const char* who = "p1_elementwise_divkgrad_diagonal_macro_3d";
   HH_REQUIRE( diag && k && macro_vertex_coords, std::string( who ) + ": null pointer" );
   HH_REQUIRE( diag != k, std::string( who ) + ": diag must not alias k" );
   Args A{};
   int  level = 0;
   int  rc    = prepare( who, macro_vertex_coords, micro_edges_per_macro_edge, A, &level );
   if ( rc != HYTEG_HIP_OK )
      return rc;
   A.dst = diag, A.src = k, A.k = k;
   rc    = launch_shell< DKG_DIAG >( A, HYTEG_HIP_MASK_SHELL, as_stream( stream ) );
   if ( rc != HYTEG_HIP_OK || level < HYTEG_HIP_MIN_LEVEL )
      return rc;
   return launch_inner_points< DKG_DIAG >( A, level, as_stream( stream ) );
}

HYTEG_HIP_API int hyteg_hip_p1_elementwise_divkgrad_set_shape( int ny, int lz )
{
   HH_REQUIRE( ( ny == 0 && lz == 0 ) || shape_compiled( Shape{ ny, lz } ), "p1_elementwise_divkgrad_set_shape: brick shape not compiled in" );
   g_shape_override = Shape{ ny, lz };
   return HYTEG_HIP_OK;
}

HYTEG_HIP_API int hyteg_hip_p1_elementwise_divkgrad_set_inner_by_points( int on )
{
   g_inner_by_points = on != 0;
   return HYTEG_HIP_OK;
}
}
