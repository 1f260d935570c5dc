// Launch layer of the variable-coefficient P1 operators (kernels_varcoef.hpp).  An operator's .hip file states what is its own in a
// struct L (p1_divkgrad.hip, p1_epsilon.hip):
//    OP                              its operator policy
//    Shapes                          the brick shapes ( rows x slices per wave ) its z-march is compiled for, a Bricks< Brick< NY, LZ >... >
//    level_shape( level )            the measured default among them
//    shape_override, inner_by_points what its two set_* entries set (tests, measurements)
#pragma once

#include <cmath>

#include "kernels_varcoef.hpp"

namespace hyteg_hip {
namespace varcoef {

constexpr int kMaxLevel = 8;

struct Shape
{
   int ny, lz;
};
template < int NY, int LZ >
struct Brick
{
   static constexpr int ny = NY, lz = LZ;
};
template < class... Bs >
struct Bricks
{
   static bool has( const Shape& s ) { return ( ( s.ny == Bs::ny && s.lz == Bs::lz ) || ... ); }
};

inline int level_of( int64_t micro_edges, int* level )
{
   if ( micro_edges < 1 || ( micro_edges & ( micro_edges - 1 ) ) != 0 )
      return HYTEG_HIP_EINVAL;
   int l = 0;
   while ( ( (int64_t) 1 << l ) < micro_edges )
      ++l;
   *level = l;
   return HYTEG_HIP_OK;
}

// validation of what every entry shares; cc: the macro-cell's vertices for the operator's weights
template < class OP >
int prepare_cell( const char* who, const double* coords, int64_t micro_edges, double ( &cc )[4][3], Args< OP >& A, int* level )
{
   const std::string w( who );
   HH_REQUIRE( coords, w + ": null pointer" );
   HH_REQUIRE( level_of( micro_edges, level ) == HYTEG_HIP_OK && *level <= kMaxLevel,
               w + ": micro_edges_per_macro_edge must be a power of two, at most 2^8" );
   for ( int v = 0; v < 4; ++v )
      for ( int r = 0; r < 3; ++r )
         cc[v][r] = coords[3 * v + r];
   double       g[4][3];
   const double V = elmat::gradients( cc, g );
   HH_REQUIRE( V > 0.0 && std::isfinite( V ), w + ": degenerate macro-cell" );
   A.N     = ( 1 << *level ) + 1;
   A.bytes = (unsigned) ( tet64( A.N ) * (int64_t) sizeof( double ) );
   return HYTEG_HIP_OK;
}

inline int shell_blocks( int N ) { return ( 4 * tri( N ) + kPointThreads - 1 ) / kPointThreads; }

template < class OP, int MODE >
int launch_shell( const Args< OP >& A, hipStream_t stream )
{
   hipLaunchKernelGGL( ( shell_kernel< OP, MODE > ), dim3( shell_blocks( A.N ) ), dim3( kPointThreads ), 0, stream, A );
   HH_CHECK_HIP( hipGetLastError() );
   return HYTEG_HIP_OK;
}

template < class OP, int MODE >
int launch_inner_points( const Args< OP >& A, int level, hipStream_t stream )
{
   TileTable tt;
   const int rc = get_tiles( level, TILES_FULL, 1024, &tt );
   if ( rc != HYTEG_HIP_OK || tt.count == 0 )
      return rc;
   hipLaunchKernelGGL( ( inner_point_kernel< OP, MODE > ), dim3( tt.count ), dim3( kPointThreads ), 0, stream, A, tt.dev, tt.count );
   HH_CHECK_HIP( hipGetLastError() );
   return HYTEG_HIP_OK;
}

// the inner points of the components in A.comps
template < class L, int MODE >
int launch_inner( const Args< typename L::OP >& A, int level, hipStream_t stream )
{
   if ( level < HYTEG_HIP_MIN_LEVEL || A.comps == 0 )
      return HYTEG_HIP_OK; // no inner points
   if ( L::inner_by_points )
      return launch_inner_points< typename L::OP, MODE >( A, level, stream );
   const Shape s = L::shape_override.ny ? L::shape_override : L::level_shape( level );
   BrickTable  bt;
   const int   rc = get_bricks( level, s.ny, s.lz, &bt );
   if ( rc != HYTEG_HIP_OK || bt.count == 0 )
      return rc;
   int nblocks         = ( bt.count + kZMarchWavesPerBlock - 1 ) / kZMarchWavesPerBlock;
   nblocks             = ( nblocks + 7 ) & ~7;
   const int xcd_chunk = nblocks / 8; // consecutive bricks on one XCD, as in the constant-stencil apply
   void ( *kernel )( const BrickTask*, int, int, Args< typename L::OP > ) = nullptr;
   [&]< class... Bs >( Bricks< Bs... > ) {
      ( ( s.ny == Bs::ny && s.lz == Bs::lz ? kernel = zmarch_kernel< typename L::OP, MODE, Bs::ny, Bs::lz > : kernel ), ... );
   }( typename L::Shapes{} );
   hipLaunchKernelGGL( kernel, dim3( nblocks ), dim3( 64 * kZMarchWavesPerBlock ), 0, stream, bt.dev, bt.count, xcd_chunk, A );
   HH_CHECK_HIP( hipGetLastError() );
   return HYTEG_HIP_OK;
}

// the body of an operator's set_shape entry; ( 0, 0 ) returns to the default
template < class L >
int set_shape( const char* who, int ny, int lz )
{
   HH_REQUIRE( ( ny == 0 && lz == 0 ) || L::Shapes::has( Shape{ ny, lz } ), std::string( who ) + ": brick shape not compiled in" );
   L::shape_override = Shape{ ny, lz };
   return HYTEG_HIP_OK;
}

} // namespace varcoef
} // namespace hyteg_hip
