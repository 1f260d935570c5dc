// C-ABI entry points of the variable-viscosity P1 epsilon operator -div( 2 mu eps(u) ) on one macro-cell: the fused form of the nine
// P1ElementwiseOperator blocks of P1ElementwiseAffineEpsilonOperator (src/mixed_operator/P1EpsilonOperator.hpp:89-164; each
// block: P1ElementwiseOperator::apply, src/hyteg/elementwiseoperators/P1ElementwiseOperator.cpp), of its extractInverseDiagonal
// (the diagonals of the three diagonal blocks) and of P1ElementwiseOperator::smooth_jac (P1ElementwiseOperator.cpp:288-331) on the
// three components.  The viscosity is a P1 function: the same operator as the reference's where mu is linear per micro-cell.
// Kernels: kernels_epsilon.hpp.
#include <cmath>

#include "device_table.hpp"
#include "kernels_epsilon.hpp"

using namespace hyteg_hip;
using namespace hyteg_hip::epsilon;

// weight form of the z-march: 0 = gradients in the kernel arguments, 1 = block products in a device table (kernels_epsilon.hpp)
#ifndef HYTEG_EPS_FORM
#define HYTEG_EPS_FORM 0
#endif

namespace {

constexpr int kMaxLevel = 8;
constexpr int kForm     = HYTEG_EPS_FORM;

// Brick shape of the z-march: rows x slices per wave.  Four operand arrays are live, so the bricks are smaller than div-k-grad's:
// every compiled shape holds its operands in registers without scratch at one wave per SIMD.  Levels <= 7 are few bricks:
// many short waves; at level 8 two rows per wave load fewer rows twice.  hyteg_hip_p1_elementwise_epsilon_set_shape overrides
// (tests, measurements).
struct Shape
{
   int ny, lz;
};
Shape g_shape_override{ 0, 0 };
#define HYTEG_EPS_SHAPES( X ) X( 1, 4 ) X( 1, 8 ) X( 2, 4 )
inline Shape shape_of( int level )
{
   if ( g_shape_override.ny )
      return g_shape_override;
   return level <= 7 ? Shape{ 1, 4 } : Shape{ 2, 4 };
}
inline bool shape_compiled( const Shape& s )
{
#define HH_X( NY_, LZ_ ) \
   if ( s.ny == NY_ && s.lz == LZ_ ) \
      return true;
   HYTEG_EPS_SHAPES( HH_X )
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

inline bool any_null( const double* const* p ) { return !p || !p[0] || !p[1] || !p[2]; }
inline bool among( const double* q, const double* const* p ) { return q == p[0] || q == p[1] || q == p[2]; }

// validation of what every entry shares, and the weights of the six micro-cell types
int prepare( const char* who, const double* coords, int64_t micro_edges, bool with_table, Args& A, int* level )
{
   const std::string w( who );
   HH_REQUIRE( coords, w + ": null pointer" );
   HH_REQUIRE( level_of( micro_edges, level ) == HYTEG_HIP_OK && *level <= kMaxLevel,
               w + ": micro_edges_per_macro_edge must be a power of two, at most 2^8" );
   double cc[4][3];
   for ( int v = 0; v < 4; ++v )
      for ( int r = 0; r < 3; ++r )
         cc[v][r] = coords[3 * v + r];
   double       g0[4][3];
   const double V0 = elmat::gradients( cc, g0 );
   HH_REQUIRE( V0 > 0.0 && std::isfinite( V0 ), w + ": degenerate macro-cell" );
   double g[6][4][3], V[6];
   for ( int t = 0; t < 6; ++t )
   {
      double c[4][3];
      elmat::micro_cell_coords( cc, micro_edges, t, c );
      V[t]           = elmat::gradients( c, g[t] );
      const double s = std::sqrt( 0.25 * V[t] );
      for ( int a = 0; a < 4; ++a )
         for ( int r = 0; r < 3; ++r )
            A.W.h[t][a][r] = s * g[t][a][r];
   }
   A.N     = ( 1 << *level ) + 1;
   A.bytes = (unsigned) ( tet64( A.N ) * (int64_t) sizeof( double ) );
   A.table = nullptr;
   if ( with_table && kForm == 1 && *level >= HYTEG_HIP_MIN_LEVEL )
   {
      std::vector< double > key( coords, coords + 12 );
      key.push_back( (double) micro_edges );
      key.push_back( 0x657073 ); // tag of this operator's tables
      return cached_operator_table(
          key,
          [&]( std::vector< double >& tab ) {
             tab.resize( kTableDoubles );
             for ( int t = 0; t < 6; ++t )
                for ( int a = 0; a < 4; ++a )
                   for ( int i = 0; i < 3; ++i )
                      for ( int j = 0; j < 3; ++j )
                         for ( int n = 0; n < 3; ++n )
                         {
                            const int    b  = ( a + 1 + n ) % 4;
                            const double gg = g[t][a][0] * g[t][b][0] + g[t][a][1] * g[t][b][1] + g[t][a][2] * g[t][b][2];
                            tab[( ( ( t * 4 + a ) * 3 + i ) * 3 + j ) * 3 + n] = 0.25 * V[t] * ( ( i == j ? gg : 0.0 ) + g[t][a][j] * g[t][b][i] );
                         }
             return HYTEG_HIP_OK;
          },
          &A.table );
   }
   return HYTEG_HIP_OK;
}

inline int shell_blocks( int N ) { return ( 4 * tri( N ) + kPointThreads - 1 ) / kPointThreads; }

template < int MODE >
int launch_shell( const Args& A, hipStream_t stream )
{
   hipLaunchKernelGGL( epsilon_shell_kernel< MODE >, dim3( shell_blocks( A.N ) ), dim3( kPointThreads ), 0, stream, A );
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
   hipLaunchKernelGGL( epsilon_inner_point_kernel< MODE >, dim3( tt.count ), dim3( kPointThreads ), 0, stream, A, tt.dev, tt.count );
   HH_CHECK_HIP( hipGetLastError() );
   return HYTEG_HIP_OK;
}

// the inner points by the one-thread-per-point kernel instead of the z-march (tests, tools/bench_kernels.py)
bool g_inner_by_points = false;

template < int MODE >
int launch_inner( const Args& A, int level, hipStream_t stream )
{
   if ( level < HYTEG_HIP_MIN_LEVEL || A.comps == 0 )
      return HYTEG_HIP_OK; // no inner points
   if ( g_inner_by_points )
      return launch_inner_points< MODE >( A, level, stream );
   const Shape s = shape_of( level );
   BrickTable  bt;
   const int   rc = get_bricks( level, s.ny, s.lz, &bt );
   if ( rc != HYTEG_HIP_OK || bt.count == 0 )
      return rc;
   int nblocks         = ( bt.count + kZMarchWavesPerBlock - 1 ) / kZMarchWavesPerBlock;
   nblocks             = ( nblocks + 7 ) & ~7;
   const int xcd_chunk = nblocks / 8; // consecutive bricks on one XCD, as in the constant-stencil apply
#define HH_X( NY_, LZ_ )                                                                                                                            \
   if ( s.ny == NY_ && s.lz == LZ_ )                                                                                                                \
      hipLaunchKernelGGL( ( epsilon_zmarch_kernel< MODE, NY_, LZ_, kForm > ), dim3( nblocks ), dim3( 64 * kZMarchWavesPerBlock ), 0, stream, bt.dev, \
                          bt.count, xcd_chunk, A );
   HYTEG_EPS_SHAPES( HH_X )
#undef HH_X
   HH_CHECK_HIP( hipGetLastError() );
   return HYTEG_HIP_OK;
}

int apply_impl( const char* who, double* const* dst, const double* const* src, const double* mu, const double* coords, int64_t micro_edges,
                const unsigned* masks, int update, hyteg_hip_stream_t stream )
{
   const std::string w( who );
   HH_REQUIRE( !any_null( dst ) && !any_null( src ) && mu && coords && masks, w + ": null pointer" );
   for ( int c = 0; c < 3; ++c )
      HH_REQUIRE( !among( dst[c], src ) && dst[c] != mu && dst[c] != dst[( c + 1 ) % 3], w + ": a dst must not alias src, mu or another dst" );
   HH_REQUIRE( update == HYTEG_HIP_REPLACE || update == HYTEG_HIP_ADD, w + ": bad update type" );
   for ( int c = 0; c < 3; ++c )
      HH_REQUIRE( ( masks[c] & ~(unsigned) HYTEG_HIP_MASK_ALL ) == 0, w + ": bad mask (15 class bits)" );
   Args A{};
   int  level = 0;
   int  rc    = prepare( who, coords, micro_edges, true, A, &level );
   if ( rc != HYTEG_HIP_OK )
      return rc;
   A.mu = mu;
   for ( int c = 0; c < 3; ++c )
   {
      A.dst[c] = dst[c], A.src[c] = src[c];
      A.masks[c] = masks[c] & HYTEG_HIP_MASK_SHELL;
      A.comps |= ( masks[c] & HYTEG_HIP_MASK_INNER ) ? ( 1u << c ) : 0u;
   }
   const bool add = update == HYTEG_HIP_ADD;
   if ( A.masks[0] | A.masks[1] | A.masks[2] )
   {
      rc = add ? launch_shell< EPS_ADD >( A, as_stream( stream ) ) : launch_shell< EPS_REPLACE >( A, as_stream( stream ) );
      if ( rc != HYTEG_HIP_OK )
         return rc;
   }
   return add ? launch_inner< EPS_ADD >( A, level, as_stream( stream ) ) : launch_inner< EPS_REPLACE >( A, level, as_stream( stream ) );
}

} // namespace

extern "C" {

HYTEG_HIP_API int hyteg_hip_p1_elementwise_epsilon_apply_macro_3d_masked( double* const*       dst,
                                                                          const double* const* src,
                                                                          const double*        mu,
                                                                          const double*        macro_vertex_coords,
                                                                          int64_t              micro_edges_per_macro_edge,
                                                                          unsigned             mask,
                                                                          int                  update,
                                                                          hyteg_hip_stream_t   stream )
{
   const unsigned masks[3] = { mask, mask, mask };
   return apply_impl( "p1_elementwise_epsilon_apply_macro_3d", dst, src, mu, macro_vertex_coords, micro_edges_per_macro_edge, masks, update, stream );
}

HYTEG_HIP_API int hyteg_hip_p1_elementwise_epsilon_apply_macro_3d_component_masks( double* const*       dst,
                                                                                   const double* const* src,
                                                                                   const double*        mu,
                                                                                   const double*        macro_vertex_coords,
                                                                                   int64_t              micro_edges_per_macro_edge,
                                                                                   const unsigned*      masks,
                                                                                   int                  update,
                                                                                   hyteg_hip_stream_t   stream )
{
   return apply_impl( "p1_elementwise_epsilon_apply_macro_3d_component_masks", dst, src, mu, macro_vertex_coords, micro_edges_per_macro_edge, masks,
                      update, stream );
}

HYTEG_HIP_API int hyteg_hip_p1_elementwise_epsilon_jacobi_macro_3d( double* const*       dst,
                                                                    const double* const* src,
                                                                    const double* const* rhs,
                                                                    const double* const* inv_diag,
                                                                    const double*        mu,
                                                                    const double*        macro_vertex_coords,
                                                                    int64_t              micro_edges_per_macro_edge,
                                                                    double               omega,
                                                                    hyteg_hip_stream_t   stream )
{
   const char* who = "p1_elementwise_epsilon_jacobi_macro_3d";
   HH_REQUIRE( !any_null( dst ) && !any_null( src ) && !any_null( rhs ) && !any_null( inv_diag ) && mu && macro_vertex_coords,
               std::string( who ) + ": null pointer" );
   for ( int c = 0; c < 3; ++c )
      HH_REQUIRE( !among( dst[c], src ) && !among( dst[c], rhs ) && !among( dst[c], inv_diag ) && dst[c] != mu && dst[c] != dst[( c + 1 ) % 3],
                  std::string( who ) + ": a dst must not alias an input or another dst" );
   Args A{};
   int  level = 0;
   int  rc    = prepare( who, macro_vertex_coords, micro_edges_per_macro_edge, true, A, &level );
   if ( rc != HYTEG_HIP_OK )
      return rc;
   A.mu = mu, A.omega = omega, A.comps = 7u;
   for ( int c = 0; c < 3; ++c )
      A.dst[c] = dst[c], A.src[c] = src[c], A.rhs[c] = rhs[c], A.invdiag[c] = inv_diag[c];
   return launch_inner< EPS_JACOBI >( A, level, as_stream( stream ) );
}

HYTEG_HIP_API int hyteg_hip_p1_elementwise_epsilon_diagonal_macro_3d( double* const*     diag,
                                                                      const double*      mu,
                                                                      const double*      macro_vertex_coords,
                                                                      int64_t            micro_edges_per_macro_edge,
                                                                      hyteg_hip_stream_t stream )
{
   const char* who = "p1_elementwise_epsilon_diagonal_macro_3d";
   HH_REQUIRE( !any_null( diag ) && mu && macro_vertex_coords, std::string( who ) + ": null pointer" );
   for ( int c = 0; c < 3; ++c )
      HH_REQUIRE( diag[c] != mu && diag[c] != diag[( c + 1 ) % 3], std::string( who ) + ": a diag must not alias mu or another diag" );
   Args A{};
   int  level = 0;
   int  rc    = prepare( who, macro_vertex_coords, micro_edges_per_macro_edge, false, A, &level );
   if ( rc != HYTEG_HIP_OK )
      return rc;
   A.mu = mu, A.comps = 7u;
   for ( int c = 0; c < 3; ++c )
      A.dst[c] = diag[c], A.src[c] = mu, A.masks[c] = HYTEG_HIP_MASK_SHELL;
   rc = launch_shell< EPS_DIAG >( A, as_stream( stream ) );
   if ( rc != HYTEG_HIP_OK || level < HYTEG_HIP_MIN_LEVEL )
      return rc;
   return launch_inner_points< EPS_DIAG >( A, level, as_stream( stream ) );
}

HYTEG_HIP_API int hyteg_hip_p1_elementwise_epsilon_set_shape( int ny, int lz )
{
   HH_REQUIRE( ( ny == 0 && lz == 0 ) || shape_compiled( Shape{ ny, lz } ), "p1_elementwise_epsilon_set_shape: brick shape not compiled in" );
   g_shape_override = Shape{ ny, lz };
   return HYTEG_HIP_OK;
}

HYTEG_HIP_API int hyteg_hip_p1_elementwise_epsilon_set_inner_by_points( int on )
{
   g_inner_by_points = on != 0;
   return HYTEG_HIP_OK;
}
}
