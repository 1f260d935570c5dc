// Launch layer of the variable-coefficient P1 operators (kernels_varcoef.hpp).  An operator's .hip file states what is its own in a
// struct L (p1_divkgrad.hip, p1_epsilon.hip):
//    OP                              its operator policy
//    Shapes                          the brick shapes ( rows x slices per wave ) its z-march is compiled for, a Bricks< Brick< NY, LZ >... >
//    compiled< MODE, NY, LZ >()      false where a mode's z-march is not compiled at a shape of Shapes (it would need scratch)
//    level_shape( level, mode )      the default among the shapes compiled for the mode
//    shape_override, inner_by_points what its two set_* entries set (tests, measurements)
#pragma once

#include <cmath>
#include <initializer_list>

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
   // an override the mode is not compiled for leaves the mode at its default
   Shape s = L::shape_override.ny ? L::shape_override : L::level_shape( level, MODE );
   void ( *kernel )( const BrickTask*, int, int, Args< typename L::OP > ) = nullptr;
   auto pick = [&]< class... Bs >( Bricks< Bs... > ) {
      (
          [&] {
             if constexpr ( L::template compiled< MODE, Bs::ny, Bs::lz >() )
                if ( s.ny == Bs::ny && s.lz == Bs::lz )
                   kernel = zmarch_kernel< typename L::OP, MODE, Bs::ny, Bs::lz >;
          }(),
          ... );
   };
   pick( typename L::Shapes{} );
   if ( !kernel )
   {
      s = L::level_shape( level, MODE );
      pick( typename L::Shapes{} );
   }
   BrickTable bt;
   const int  rc = get_bricks( level, s.ny, s.lz, &bt );
   if ( rc != HYTEG_HIP_OK || bt.count == 0 )
      return rc;
   int nblocks         = ( bt.count + kZMarchWavesPerBlock - 1 ) / kZMarchWavesPerBlock;
   nblocks             = ( nblocks + 7 ) & ~7;
   const int xcd_chunk = nblocks / 8; // consecutive bricks on one XCD, as in the constant-stencil apply
   hipLaunchKernelGGL( kernel, dim3( nblocks ), dim3( 64 * kZMarchWavesPerBlock ), 0, stream, bt.dev, bt.count, xcd_chunk, A );
   HH_CHECK_HIP( hipGetLastError() );
   return HYTEG_HIP_OK;
}

// ---- the fused residual and Chebyshev entries (inner points only).  An argument is an array of NC pointers; prepare is the
// operator's own validation and weights.  A written array must differ from every other array of the call, and nothing aliases the
// coefficient. ----
template < int NC >
bool null_in( const double* const* p )
{
   if ( !p )
      return true;
   for ( int c = 0; c < NC; ++c )
      if ( !p[c] )
         return true;
   return false;
}

template < int NC >
bool arrays_distinct( std::initializer_list< const double* const* > written, std::initializer_list< const double* const* > read, const double* coef )
{
   // at most two written and three read arguments of NC pointers each: on the stack, this runs once per cell and step
   const double* w[2 * NC];
   const double* r[3 * NC];
   int           nw = 0, nr = 0;
   for ( auto a : written )
      for ( int c = 0; c < NC; ++c )
         w[nw++] = a[c];
   for ( auto a : read )
      for ( int c = 0; c < NC; ++c )
         r[nr++] = a[c];
   for ( int i = 0; i < nw; ++i )
   {
      if ( w[i] == coef )
         return false;
      for ( int j = 0; j < i; ++j )
         if ( w[i] == w[j] )
            return false;
      for ( int j = 0; j < nr; ++j )
         if ( w[i] == r[j] )
            return false;
   }
   for ( int j = 0; j < nr; ++j )
      if ( r[j] == coef )
         return false;
   return true;
}

// dst = rhs - A src ( START == false ),  dst = inv_diag .* ( rhs - A src ) ( START == true; dst is t_out and src is x )
template < class L, bool START, class Prepare >
int residual_entry( const char* who, Prepare prepare, double* const* dst, const double* const* src, const double* const* rhs,
                    const double* const* inv_diag, const double* coef, const double* coords, int64_t micro_edges, unsigned comps, hipStream_t stream )
{
   constexpr int     NC = L::OP::NC;
   const std::string w( who );
   HH_REQUIRE( !null_in< NC >( dst ) && !null_in< NC >( src ) && !null_in< NC >( rhs ) && ( !START || !null_in< NC >( inv_diag ) ) && coef && coords,
               w + ": null pointer" );
   HH_REQUIRE( ( comps >> NC ) == 0, w + ": bad component bits" );
   HH_REQUIRE( START ? arrays_distinct< NC >( { dst }, { src, rhs, inv_diag }, coef ) : arrays_distinct< NC >( { dst }, { src, rhs }, coef ),
               w + ": a dst must not alias an input or another dst, and nothing the coefficient" );
   Args< typename L::OP > A{};
   int                    level = 0;
   const int              rc    = prepare( who, coords, micro_edges, A, &level );
   if ( rc != HYTEG_HIP_OK )
      return rc;
   A.coef = coef, A.comps = comps;
   for ( int c = 0; c < NC; ++c )
   {
      A.dst[c] = dst[c], A.src[c] = src[c], A.rhs[c] = rhs[c];
      if ( START )
         A.invdiag[c] = inv_diag[c];
   }
   return START ? launch_inner< L, CHEB_START >( A, level, stream ) : launch_inner< L, RESIDUAL >( A, level, stream );
}

// t_out = inv_diag .* ( A t_in ),  x = ( x + c_prev t_in ) + c_cur t_out, the first summand only if has_prev
template < class L, class Prepare >
int chebyshev_step_entry( const char* who, Prepare prepare, double* const* t_out, double* const* x, const double* const* t_in,
                          const double* const* inv_diag, const double* coef, const double* coords, int64_t micro_edges, double c_prev, double c_cur,
                          int has_prev, unsigned comps, hipStream_t stream )
{
   constexpr int     NC = L::OP::NC;
   const std::string w( who );
   HH_REQUIRE( !null_in< NC >( t_out ) && !null_in< NC >( x ) && !null_in< NC >( t_in ) && !null_in< NC >( inv_diag ) && coef && coords,
               w + ": null pointer" );
   HH_REQUIRE( ( comps >> NC ) == 0, w + ": bad component bits" );
   HH_REQUIRE( arrays_distinct< NC >( { t_out, x }, { t_in, inv_diag }, coef ),
               w + ": t_out, x and t_in must not alias each other or inv_diag, and nothing the coefficient" );
   Args< typename L::OP > A{};
   int                    level = 0;
   const int              rc    = prepare( who, coords, micro_edges, A, &level );
   if ( rc != HYTEG_HIP_OK )
      return rc;
   A.coef = coef, A.comps = comps, A.cPrev = c_prev, A.cCur = c_cur, A.hasPrev = has_prev != 0;
   for ( int c = 0; c < NC; ++c )
      A.dst[c] = t_out[c], A.x[c] = x[c], A.src[c] = t_in[c], A.invdiag[c] = inv_diag[c];
   return launch_inner< L, CHEB_STEP >( A, level, stream );
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
