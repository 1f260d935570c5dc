// C-ABI entry points: constant-stencil apply and fused weighted Jacobi on one macro-cell.
#include <cstdlib>
#include <string>
#include <type_traits>

#include "kernels_apply.hpp"
#include "kernels_apply_zmarch.hpp"

using namespace hyteg_hip;

namespace {

constexpr int kTile = 1024;

// Brick shape of the z-march kernel: rows x slices per wave, and how many slices the loads run ahead of the arithmetic.
// The shape trades reuse (taller / wider bricks re-read fewer halo rows and slices) against the number of waves and against the
// share of a wave's loads that precede its first store (the prologue: (2 + PFD) of LZ + 2 slices).
struct BrickShape
{
   int  ny, lz, pfd;
   bool operator==( const BrickShape& o ) const { return ny == o.ny && lz == o.lz && pfd == o.pfd; }
};
BrickShape g_shape_override{ 0, 0, 0 }; // hyteg_hip_set_apply_shape (tuning knob; 0 = the defaults below)

// Defaults read off the sweep of every compiled shape x mode x level (tools/apply_shape_sweep.py) with every operand class 2.2 x
// larger than the Infinity Cache (HBM regime, profiles/r03_apply_shape_sweep_hbm.txt).  Levels <= 7 (a few hundred bricks, arrays
// of a few MB: cache-resident in any cycle) want many short waves.  Level 8 (one generation of waves, HBM-bound) wants 4 x 8, two
// slices ahead, and one slice ahead for the modes that read a second array and store one (Add, residual: 16.6 against 17.2 /
// 17.3 us); everything taller or wider is slower (6 x 8: 15.3, 4 x 16: 17.3 us against 12.2-12.55).  From level 9 on (several
// generations, HBM either way) 4 x 4, two ahead.  The first sweep of round 3 (profiles/r03_apply_shape_sweep.txt) ran on rings
// whose SOURCE arrays fitted into the Infinity Cache and preferred 2 x 8, one slice ahead, for level-8 Replace (9.15 against
// 9.50 us); read from HBM that shape is the slower one (13.3 against 12.5 us).
// All of this is the SINGLE launch (one generation of at most 2048 waves that start together); it is also the form of a steps
// launch wherever steps_shape below says nothing else.
inline BrickShape default_shape( int mode, int level, bool f32 )
{
   if ( level <= 7 )
      return ( mode == APPLY_REPLACE || f32 ) ? BrickShape{ 2, 4, 1 } : BrickShape{ 4, 4, 1 };
   if ( level == 8 )
      return ( mode == APPLY_ADD || mode == APPLY_RESIDUAL ) ? BrickShape{ 4, 8, 1 } : BrickShape{ 4, 8, 2 };
   return BrickShape{ 4, 4, 2 };
}

// the shapes compiled in: the defaults (6 x 8: the steps launch) and the runners-up of the sweep (so that the sweep can be
// repeated on another box)
#define HYTEG_ZM_SHAPES( X ) X( 2, 8, 1 ) X( 4, 8, 2 ) X( 4, 8, 1 ) X( 4, 4, 2 ) X( 4, 4, 1 ) X( 2, 4, 1 ) X( 8, 4, 2 ) X( 6, 8, 2 )

// run-time shape -> compile-time ( NY, LZ, PFD ): calls f with the three as std::integral_constant arguments if s is compiled
// in and says whether it is.  The one expansion of HYTEG_ZM_SHAPES.
template < typename F >
bool with_compiled_shape( const BrickShape& s, F&& f )
{
#define HH_X( NY_, LZ_, PFD_ ) \
   if ( s == BrickShape{ NY_, LZ_, PFD_ } ) \
      return f( std::integral_constant< int, NY_ >{}, std::integral_constant< int, LZ_ >{}, std::integral_constant< int, PFD_ >{} ), true;
   HYTEG_ZM_SHAPES( HH_X )
#undef HH_X
   return false;
}

inline bool shape_compiled( const BrickShape& s )
{
   return with_compiled_shape( s, []( auto, auto, auto ) {} );
}

// the shape of a launch: hyteg_hip_set_apply_shape, else HYTEG_HIP_APPLY_SHAPE=NYxLZxPFD from the environment (read once;
// lets tools/gpu/r03_shapes.sh A/B whole bench.py runs), else the default of the mode and level
inline bool overridden_shape( BrickShape& s )
{
   static const BrickShape env = [] {
      BrickShape  e{ 0, 0, 0 };
      const char* v = getenv( "HYTEG_HIP_APPLY_SHAPE" );
      if ( v && sscanf( v, "%dx%dx%d", &e.ny, &e.lz, &e.pfd ) != 3 )
         e = BrickShape{ -1, -1, -1 }; // unparsable: every launch fails with "not compiled in"
      return e;
   }();
   if ( g_shape_override.ny )
      return s = g_shape_override, true;
   if ( env.ny )
      return s = env, true;
   return false;
}
inline BrickShape current_shape( int mode, int level, bool f32 )
{
   BrickShape s;
   return overridden_shape( s ) ? s : default_shape( mode, level, f32 );
}

// The steps launch has a form of its own: brick shape and x-stride (62: plain row segments; 56: store windows aligned to the
// 64-byte lines of dst, kernels_apply_zmarch.hpp).  Its bricks stream through the wave slots without a common start, so the
// wave count of one apply is not tied to the slot count and the reasons for 4 x 8 above (one generation of ~2000 waves) do not
// hold.  Level-8 Replace, groups of 13 on two lanes, one bench.py run each (profiles/apply_steps_shapes_level8.txt):
//            4x8/2   8x8/2   8x8/3   6x8/2   4x8/3    parent
//   XS 62    9.50    9.79    9.78    9.83    9.35     9.37 .. 9.53
//   XS 56    9.25    9.28    9.55    9.20    9.48
// Taller bricks lose on their own (fewer, longer waves), aligned windows gain nothing on their own (4 x 8: 9.19-9.23 against
// 9.18-9.35 us in the alternating rounds); together they win: 6 x 8 and 8 x 8, two ahead, 56 wide, 8.90-9.03 us.  The other
// modes and levels keep the shape of the single apply, 62 wide (Add was not measured; levels <= 7 are cache-resident).
// Overrides keep priority: the shape of hyteg_hip_set_apply_shape / HYTEG_HIP_APPLY_SHAPE, the x-stride of
// hyteg_hip_set_apply_steps_xs / HYTEG_HIP_APPLY_STEPS_XS (read once).
struct StepsForm
{
   BrickShape shape;
   int        xs;
};
int g_steps_xs_override = 0; // hyteg_hip_set_apply_steps_xs (tuning knob; 0 = the default of the mode and level)

inline StepsForm steps_shape( int mode, int level )
{
   static const int envXs = [] {
      const char* v = getenv( "HYTEG_HIP_APPLY_STEPS_XS" );
      return v ? atoi( v ) : 0;
   }();
   StepsForm f = ( level == 8 && mode == APPLY_REPLACE ) ? StepsForm{ BrickShape{ 6, 8, 2 }, 56 } : StepsForm{ default_shape( mode, level, false ), 62 };
   overridden_shape( f.shape );
   if ( g_steps_xs_override )
      f.xs = g_steps_xs_override;
   else if ( envXs )
      f.xs = envXs;
   return f;
}

// what every z-march launch of a level and shape carries whatever its arrays: brick table, extents, stencil, XCD slab map.
// nblocks = 0 on return: no bricks, nothing to launch
template < typename T >
int zmarch_common_args( ZMarchArgs& A, int& nblocks, int NY, int LZ, int level, const double* w, int XS = 62 )
{
   nblocks = 0;
   BrickTable bt;
   int        rc = get_bricks( level, NY, LZ, &bt, XS );
   if ( rc != HYTEG_HIP_OK || bt.count == 0 )
      return rc;
   A.tasks  = bt.dev;
   A.ntasks = bt.count;
   A.N      = ( 1 << level ) + 1;
   A.bytes  = (unsigned) ( tet64( A.N ) * (int64_t) sizeof( T ) );
   for ( int k = 0; k < 15; ++k )
      A.st.w[k] = w[k];
   nblocks     = ( bt.count + kZMarchWavesPerBlock - 1 ) / kZMarchWavesPerBlock;
   nblocks     = ( nblocks + 7 ) & ~7;
   A.xcd_chunk = nblocks / 8;
   // measurement switch: 0 = workgroups in launch order (XCDs interleaved brick by brick)
   static const bool xcdSlabs = env_flag( "HYTEG_HIP_APPLY_XCD_SLABS", true );
   if ( !xcdSlabs )
      A.xcd_chunk = 0;
   return HYTEG_HIP_OK;
}

// `extra`: the second float output of APPLY_RESIDUAL_F32OUT / the double accumulator of APPLY_JACOBI_ACCUM / the iterate of APPLY_CHEB_STEP
// (whose deferred update is relax2, applied if flag != 0)
template < int MODE, int NY, int LZ, int PFD, typename T >
int launch_zmarch_shape( void* dst, const T* src, const T* rhs, const T* invdiag, int level, const double* w, double relax, hipStream_t stream,
                         void* extra, double relax2, int flag )
{
   ZMarchArgs A{};
   int        nblocks = 0;
   const int  rc      = zmarch_common_args< T >( A, nblocks, NY, LZ, level, w );
   if ( rc != HYTEG_HIP_OK || nblocks == 0 )
      return rc;
   A.dst     = dst;
   A.src     = src;
   A.rhs     = rhs;
   A.invdiag = invdiag;
   A.dst2    = extra;
   A.xacc    = static_cast< double* >( extra );
   A.relax   = relax;
   A.relax2  = relax2;
   A.flag    = flag;
   // the first three arguments are preloaded into SGPRs (-mllvm -amdgpu-kernarg-preload-count=4): the task load does not wait
   // for a kernel-argument load (round 2: 9.90-10.18 -> 9.60-9.74 us)
   hipLaunchKernelGGL( ( p1_apply_zmarch_preload_kernel< MODE, NY, LZ, PFD, T > ), dim3( nblocks ), dim3( 64 * kZMarchWavesPerBlock ), 0, stream, A.tasks,
                       A.ntasks, A.xcd_chunk, A );
   HH_CHECK_HIP( hipGetLastError() );
   return HYTEG_HIP_OK;
}

// Residency cap of the steps launch: m workgroups per CU (m waves per SIMD) by a request for dynamic LDS the kernel never touches --
// 160 KiB / m per workgroup, rounded down to 4 KiB, so that m workgroups fit a CU's LDS and m + 1 do not (m = 1 .. 6).  Without
// a cap up to 8 waves per SIMD are resident, i.e. the working sets of up to four steps share an L2.  Default: m = 2 at level 8
// (HBM regime: faster than no cap in nine of nine pairs of runs, -1 to -7 %), no cap below (cache-resident: m = 2 costs +16 % at
// level 7, +2 to +20 % at level 6); profiles/apply_steps_level8.txt.  The host layer issues no steps launch above level 8.
// HYTEG_HIP_APPLY_STEPS_WG_PER_CU (read once) sets m for every level; 0 or out of range: no cap.
inline unsigned steps_lds_request( int level )
{
   static const int fromEnv = [] {
      const char* v = getenv( "HYTEG_HIP_APPLY_STEPS_WG_PER_CU" );
      return v ? atoi( v ) : -1;
   }();
   const int m = fromEnv >= 0 ? fromEnv : ( level == 8 ? 2 : 0 );
   return ( m >= 1 && m <= 6 ) ? (unsigned) ( ( 160 * 1024 / m ) & ~4095 ) : 0u;
}

// nsteps (2 .. kZMarchMaxSteps) independent applies of one stencil in one launch, double Replace / Add
template < int MODE, int NY, int LZ, int PFD, int XS >
int launch_zmarch_steps_shape( void* const* dsts, const void* const* srcs, int nsteps, int level, const double* w, hipStream_t stream )
{
   static_assert( MODE == APPLY_REPLACE || MODE == APPLY_ADD, "steps launch: Replace and Add" );
   ZMarchArgs A{};
   int        nblocks = 0;
   const int  rc      = zmarch_common_args< double >( A, nblocks, NY, LZ, level, w, XS );
   if ( rc != HYTEG_HIP_OK || nblocks == 0 )
      return rc;
   ZMarchStepPtrs P{};
   for ( int k = 0; k < kZMarchMaxSteps; ++k ) // the entries past nsteps repeat step 0: no wave reads them, none is null
   {
      P.srcs[k] = srcs[k < nsteps ? k : 0];
      P.dsts[k] = dsts[k < nsteps ? k : 0];
   }
   A.src = P.srcs[0];
   A.dst = P.dsts[0];
   auto           kern = p1_apply_zmarch_steps_kernel< MODE, NY, LZ, PFD, double, XS >;
   const unsigned lds  = steps_lds_request( level );
   if ( lds > 0 )
   {
      static const hipError_t attr = hipFuncSetAttribute( reinterpret_cast< const void* >( kern ), hipFuncAttributeMaxDynamicSharedMemorySize, (int) lds );
      HH_CHECK_HIP( attr );
   }
   hipLaunchKernelGGL( kern, dim3( nblocks, nsteps ), dim3( 64 * kZMarchWavesPerBlock ), lds, stream, A.tasks, A.ntasks, A.xcd_chunk, A, P );
   HH_CHECK_HIP( hipGetLastError() );
   return HYTEG_HIP_OK;
}

template < int MODE, typename T = double >
int launch_zmarch( void* dst, const T* src, const T* rhs, const T* invdiag, int level, const double* w, double relax, hipStream_t stream,
                   void* extra = nullptr, double relax2 = 0.0, int flag = 0 )
{
   // the fused mixed-precision steps take the shapes of the kernels they replace (residual / float Jacobi); the Chebyshev steps
   // stream three / four arrays like the Jacobi sweep and take its shapes
   const int shapeMode = MODE == APPLY_RESIDUAL_F32OUT ? APPLY_RESIDUAL :
                                                         ( ( MODE == APPLY_JACOBI_ACCUM || MODE == APPLY_CHEB_START || MODE == APPLY_CHEB_STEP ) ? APPLY_JACOBI : MODE );
   int        rc       = HYTEG_HIP_OK;
   const bool compiled = with_compiled_shape( current_shape( shapeMode, level, !std::is_same< T, double >::value ), [&]( auto ny, auto lz, auto pfd ) {
      rc = launch_zmarch_shape< MODE, decltype( ny )::value, decltype( lz )::value, decltype( pfd )::value, T >( dst, src, rhs, invdiag, level, w, relax, stream,
                                                                                                                 extra, relax2, flag );
   } );
   return compiled ? rc : fail( HYTEG_HIP_EINVAL, "apply: brick shape not compiled in" );
}

template < int MODE >
int launch_zmarch_steps( void* const* dsts, const void* const* srcs, int nsteps, int level, const double* w, hipStream_t stream )
{
   int        rc       = HYTEG_HIP_OK;
   const StepsForm form     = steps_shape( MODE, level );
   const bool      compiled = ( form.xs == 56 || form.xs == 62 ) && with_compiled_shape( form.shape, [&]( auto ny, auto lz, auto pfd ) {
      if ( form.xs == 56 )
         rc = launch_zmarch_steps_shape< MODE, decltype( ny )::value, decltype( lz )::value, decltype( pfd )::value, 56 >( dsts, srcs, nsteps, level, w, stream );
      else
         rc = launch_zmarch_steps_shape< MODE, decltype( ny )::value, decltype( lz )::value, decltype( pfd )::value, 62 >( dsts, srcs, nsteps, level, w, stream );
   } );
   return compiled ? rc : fail( HYTEG_HIP_EINVAL, "apply steps: brick shape or x-stride not compiled in" );
}

// Does this level run the z-march register kernel?  Yes whenever the byte offsets of the array fit its 32-bit buffer addressing
// (level <= 10); level 11 takes the LDS-tiled kernel (pointer addressing) and the composed Chebyshev steps.
// HYTEG_HIP_APPLY_LDS_TILED=1 (read once) sends every level down the level-11 paths, so that they can be tested entry by entry at small
// levels.  The one predicate of launch_apply, the two Chebyshev entry points and hyteg_hip_p1_apply_kernel_name; the entry points
// without a tiled form (_f32, p1_residual_cell, the mixed-precision steps) do not ask it and keep the z-march.
inline bool level_runs_zmarch( int level )
{
   static const bool forceTiled = env_flag( "HYTEG_HIP_APPLY_LDS_TILED", false );
   return !forceTiled && tet64( ( 1 << level ) + 1 ) * 8 < ( (int64_t) 1 << 31 );
}

template < int MODE >
int launch_apply( double* dst, const double* src, const double* rhs, const double* invdiag, int level, const double* w,
                  double relax, hipStream_t stream )
{
   if ( level_runs_zmarch( level ) )
      return launch_zmarch< MODE >( dst, src, rhs, invdiag, level, w, relax, stream );

   TileTable tt;
   int       rc = get_tiles( level, TILES_INNER, kTile, &tt );
   if ( rc != HYTEG_HIP_OK )
      return rc;
   if ( tt.count == 0 )
      return HYTEG_HIP_OK;

   ApplyArgs A;
   A.dst     = dst;
   A.src     = src;
   A.rhs     = rhs;
   A.invdiag = invdiag;
   A.tiles   = tt.dev;
   A.ntiles  = tt.count;
   A.N       = ( 1 << level ) + 1;
   A.total   = (int) tet64( A.N );
   A.relax   = relax;
   for ( int k = 0; k < 15; ++k )
      A.st.w[k] = w[k];
   const int nblocks = ( tt.count + 7 ) & ~7;
   A.xcd_chunk       = nblocks / 8;

   const size_t lds_bytes = (size_t) apply_lds_doubles( kTile, A.N ) * sizeof( double );
   const bool   vec       = ( reinterpret_cast< uintptr_t >( src ) & 15 ) == 0;
   auto         kern      = vec ? p1_apply_tiled_kernel< MODE, true > : p1_apply_tiled_kernel< MODE, false >;
   if ( lds_bytes > 48 * 1024 )
      HH_CHECK_HIP( hipFuncSetAttribute( reinterpret_cast< const void* >( kern ),
                                         hipFuncAttributeMaxDynamicSharedMemorySize,
                                         (int) lds_bytes ) );
   hipLaunchKernelGGL( kern, dim3( nblocks ), dim3( kApplyThreads ), lds_bytes, stream, A );
   HH_CHECK_HIP( hipGetLastError() );
   return HYTEG_HIP_OK;
}

} // namespace

extern "C" {

HYTEG_HIP_API int hyteg_hip_p1_apply_cell( double*            dst,
                                           const double*      src,
                                           int                level,
                                           const double*      w,
                                           int                update,
                                           hyteg_hip_stream_t stream )
{
   HH_REQUIRE( dst && src && w, "p1_apply_cell: null pointer" );
   HH_REQUIRE( level_ok( level ), "p1_apply_cell: level out of range [2,11]" );
   HH_REQUIRE( dst != src, "p1_apply_cell: src and dst must not alias" );
   HH_REQUIRE( update == HYTEG_HIP_REPLACE || update == HYTEG_HIP_ADD, "p1_apply_cell: bad update type" );
   if ( update == HYTEG_HIP_REPLACE )
      return launch_apply< APPLY_REPLACE >( dst, src, nullptr, nullptr, level, w, 0.0, as_stream( stream ) );
   return launch_apply< APPLY_ADD >( dst, src, nullptr, nullptr, level, w, 0.0, as_stream( stream ) );
}

HYTEG_HIP_API int hyteg_hip_p1_apply_cell_steps( void* const*       dsts,
                                                 const void* const* srcs,
                                                 int                nsteps,
                                                 int                level,
                                                 const double*      w,
                                                 int                update,
                                                 hyteg_hip_stream_t stream )
{
   HH_REQUIRE( dsts && srcs && w, "p1_apply_cell_steps: null pointer" );
   HH_REQUIRE( nsteps >= 1 && nsteps <= kZMarchMaxSteps, "p1_apply_cell_steps: nsteps out of range [1,16]" );
   HH_REQUIRE( level_ok( level ), "p1_apply_cell_steps: level out of range [2,11]" );
   HH_REQUIRE( update == HYTEG_HIP_REPLACE || update == HYTEG_HIP_ADD, "p1_apply_cell_steps: bad update type" );
   for ( int i = 0; i < nsteps; ++i )
   {
      HH_REQUIRE( dsts[i] && srcs[i], "p1_apply_cell_steps: null array" );
      for ( int j = 0; j < nsteps; ++j )
         HH_REQUIRE( dsts[i] != srcs[j] && ( i == j || dsts[i] != dsts[j] ),
                     "p1_apply_cell_steps: an array written by one step must not be read or written by another (nor be the step's own source)" );
   }
   if ( nsteps == 1 )
      return hyteg_hip_p1_apply_cell( static_cast< double* >( dsts[0] ), static_cast< const double* >( srcs[0] ), level, w, update, stream );
   if ( !level_runs_zmarch( level ) )
      return fail( HYTEG_HIP_ENOTSUP, "p1_apply_cell_steps: this level does not run the z-march kernel" );
   if ( update == HYTEG_HIP_REPLACE )
      return launch_zmarch_steps< APPLY_REPLACE >( dsts, srcs, nsteps, level, w, as_stream( stream ) );
   return launch_zmarch_steps< APPLY_ADD >( dsts, srcs, nsteps, level, w, as_stream( stream ) );
}

// ---- float instantiations (the reference instantiates its generated apply kernels for float as well:
// apply_3D_macrocell_vertexdof_to_vertexdof_replace.cpp:96-97); levels 2..10 (32-bit buffer addressing) ----
HYTEG_HIP_API int hyteg_hip_p1_apply_cell_f32( float* dst, const float* src, int level, const double* w, int update, hyteg_hip_stream_t stream )
{
   HH_REQUIRE( dst && src && w, "p1_apply_cell_f32: null pointer" );
   HH_REQUIRE( level >= HYTEG_HIP_MIN_LEVEL && level <= 10, "p1_apply_cell_f32: level out of range [2,10]" );
   HH_REQUIRE( dst != src, "p1_apply_cell_f32: src and dst must not alias" );
   HH_REQUIRE( update == HYTEG_HIP_REPLACE || update == HYTEG_HIP_ADD, "p1_apply_cell_f32: bad update type" );
   if ( update == HYTEG_HIP_REPLACE )
      return launch_zmarch< APPLY_REPLACE, float >( dst, src, nullptr, nullptr, level, w, 0.0, as_stream( stream ) );
   return launch_zmarch< APPLY_ADD, float >( dst, src, nullptr, nullptr, level, w, 0.0, as_stream( stream ) );
}

HYTEG_HIP_API int hyteg_hip_p1_jacobi_cell_f32( float*             dst,
                                                const float*       rhs,
                                                const float*       src,
                                                const float*       invdiag,
                                                int                level,
                                                const double*      w,
                                                double             relax,
                                                hyteg_hip_stream_t stream )
{
   HH_REQUIRE( dst && rhs && src && w, "p1_jacobi_cell_f32: null pointer" );
   HH_REQUIRE( level >= HYTEG_HIP_MIN_LEVEL && level <= 10, "p1_jacobi_cell_f32: level out of range [2,10]" );
   HH_REQUIRE( dst != src, "p1_jacobi_cell_f32: src and dst must not alias" );
   HH_REQUIRE( w[7] != 0.0, "p1_jacobi_cell_f32: zero centre weight" );
   return launch_zmarch< APPLY_JACOBI, float >( dst, src, rhs, invdiag, level, w, relax, as_stream( stream ) );
}

HYTEG_HIP_API int hyteg_hip_p1_residual_cell( double*            dst,
                                              const double*      rhs,
                                              const double*      src,
                                              int                level,
                                              const double*      w,
                                              hyteg_hip_stream_t stream )
{
   HH_REQUIRE( dst && rhs && src && w, "p1_residual_cell: null pointer" );
   HH_REQUIRE( level >= HYTEG_HIP_MIN_LEVEL && level <= 10, "p1_residual_cell: level out of range [2,10]" );
   HH_REQUIRE( dst != src, "p1_residual_cell: src and dst must not alias" );
   return launch_zmarch< APPLY_RESIDUAL >( dst, src, rhs, (const double*) nullptr, level, w, 0.0, as_stream( stream ) );
}

// ---- the two fused steps of the mixed-precision Jacobi smoother (host/solvers.hpp MixedPrecisionJacobiSmoother::solveSteps) ----
HYTEG_HIP_API int hyteg_hip_p1_residual_jacobi_start_f32( float*             r_f32,
                                                          float*             e_f32,
                                                          const double*      rhs,
                                                          const double*      src,
                                                          int                level,
                                                          const double*      w,
                                                          double             relax,
                                                          hyteg_hip_stream_t stream )
{
   HH_REQUIRE( r_f32 && e_f32 && rhs && src && w, "p1_residual_jacobi_start_f32: null pointer" );
   HH_REQUIRE( level >= HYTEG_HIP_MIN_LEVEL && level <= 10, "p1_residual_jacobi_start_f32: level out of range [2,10]" );
   HH_REQUIRE( r_f32 != e_f32, "p1_residual_jacobi_start_f32: the two outputs must differ" );
   HH_REQUIRE( w[7] != 0.0, "p1_residual_jacobi_start_f32: zero centre weight" );
   return launch_zmarch< APPLY_RESIDUAL_F32OUT >( r_f32, src, rhs, (const double*) nullptr, level, w, relax, as_stream( stream ), e_f32 );
}

HYTEG_HIP_API int hyteg_hip_p1_jacobi_accumulate_f32( double*            x,
                                                      const float*       rhs_f32,
                                                      const float*       e_f32,
                                                      int                level,
                                                      const double*      w,
                                                      double             relax,
                                                      hyteg_hip_stream_t stream )
{
   HH_REQUIRE( x && rhs_f32 && e_f32 && w, "p1_jacobi_accumulate_f32: null pointer" );
   HH_REQUIRE( level >= HYTEG_HIP_MIN_LEVEL && level <= 10, "p1_jacobi_accumulate_f32: level out of range [2,10]" );
   HH_REQUIRE( w[7] != 0.0, "p1_jacobi_accumulate_f32: zero centre weight" );
   return launch_zmarch< APPLY_JACOBI_ACCUM, float >( nullptr, e_f32, rhs_f32, (const float*) nullptr, level, w, relax, as_stream( stream ), x );
}

// ---- the two fused steps of the Chebyshev smoother (host/chebyshev.hpp ChebyshevSmoother::solve) ----
// A level that does not run the z-march (level_runs_zmarch: level 11, or every level under HYTEG_HIP_APPLY_LDS_TILED=1) composes the step
// from the entry points it fuses.
HYTEG_HIP_API int hyteg_hip_p1_chebyshev_start_cell( double*            t_out,
                                                     const double*      rhs,
                                                     const double*      x,
                                                     const double*      invdiag,
                                                     int                level,
                                                     const double*      w,
                                                     hyteg_hip_stream_t stream )
{
   HH_REQUIRE( t_out && rhs && x && w, "p1_chebyshev_start_cell: null pointer" );
   HH_REQUIRE( level_ok( level ), "p1_chebyshev_start_cell: level out of range [2,11]" );
   HH_REQUIRE( t_out != x && t_out != rhs && t_out != invdiag, "p1_chebyshev_start_cell: t_out must not alias x, rhs or invdiag" );
   HH_REQUIRE( w[7] != 0.0, "p1_chebyshev_start_cell: zero centre weight" );
   if ( level_runs_zmarch( level ) )
      return launch_zmarch< APPLY_CHEB_START >( t_out, x, rhs, invdiag, level, w, 0.0, as_stream( stream ) );
   int rc = hyteg_hip_p1_apply_cell( t_out, x, level, w, HYTEG_HIP_REPLACE, stream );
   if ( rc != HYTEG_HIP_OK )
      return rc;
   const double* diff[2] = { rhs, t_out };
   const double  pm[2]   = { 1.0, -1.0 };
   rc                    = hyteg_hip_p1_assign_cell( t_out, 2, diff, pm, level, stream );
   if ( rc != HYTEG_HIP_OK )
      return rc;
   if ( invdiag )
   {
      const double* prod[2] = { invdiag, t_out };
      return hyteg_hip_p1_mult_cell( t_out, 2, prod, level, stream );
   }
   const double* one[1] = { t_out };
   const double  inv[1] = { 1.0 / w[7] };
   return hyteg_hip_p1_assign_cell( t_out, 1, one, inv, level, stream );
}

HYTEG_HIP_API int hyteg_hip_p1_chebyshev_step_cell( double*            t_out,
                                                    double*            x,
                                                    const double*      t_in,
                                                    const double*      invdiag,
                                                    int                level,
                                                    const double*      w,
                                                    double             c_prev,
                                                    double             c_cur,
                                                    int                has_prev,
                                                    hyteg_hip_stream_t stream )
{
   HH_REQUIRE( t_out && x && t_in && w, "p1_chebyshev_step_cell: null pointer" );
   HH_REQUIRE( level_ok( level ), "p1_chebyshev_step_cell: level out of range [2,11]" );
   HH_REQUIRE( t_out != t_in && t_out != x && x != t_in, "p1_chebyshev_step_cell: t_out, x and t_in must be three different arrays" );
   HH_REQUIRE( invdiag != t_out && invdiag != x, "p1_chebyshev_step_cell: invdiag must not alias an output" );
   HH_REQUIRE( w[7] != 0.0, "p1_chebyshev_step_cell: zero centre weight" );
   if ( level_runs_zmarch( level ) )
      return launch_zmarch< APPLY_CHEB_STEP >( t_out, t_in, (const double*) nullptr, invdiag, level, w, c_cur, as_stream( stream ), x, c_prev,
                                               has_prev ? 1 : 0 );
   int rc = hyteg_hip_p1_apply_cell( t_out, t_in, level, w, HYTEG_HIP_REPLACE, stream );
   if ( rc != HYTEG_HIP_OK )
      return rc;
   if ( invdiag )
   {
      const double* prod[2] = { invdiag, t_out };
      rc                    = hyteg_hip_p1_mult_cell( t_out, 2, prod, level, stream );
   }
   else
   {
      const double* one[1] = { t_out };
      const double  inv[1] = { 1.0 / w[7] };
      rc                   = hyteg_hip_p1_assign_cell( t_out, 1, one, inv, level, stream );
   }
   if ( rc != HYTEG_HIP_OK )
      return rc;
   if ( has_prev )
   {
      const double* s[1] = { t_in };
      rc                 = hyteg_hip_p1_add_cell( x, 1, s, &c_prev, level, stream );
      if ( rc != HYTEG_HIP_OK )
         return rc;
   }
   const double* s[1] = { t_out };
   return hyteg_hip_p1_add_cell( x, 1, s, &c_cur, level, stream );
}

HYTEG_HIP_API int hyteg_hip_p1_apply_kernel_name( int level, int update, char* buf, size_t buflen )
{
   HH_REQUIRE( buf && buflen > 0, "p1_apply_kernel_name: null buffer" );
   HH_REQUIRE( level_ok( level ), "p1_apply_kernel_name: level out of range [2,11]" );
   HH_REQUIRE( update == HYTEG_HIP_REPLACE || update == HYTEG_HIP_ADD, "p1_apply_kernel_name: bad update type" );
   const int mode = update == HYTEG_HIP_REPLACE ? APPLY_REPLACE : APPLY_ADD;
   if ( !level_runs_zmarch( level ) )
   {
      snprintf( buf, buflen, "p1_apply_tiled_kernel<MODE=%d>", mode );
      return HYTEG_HIP_OK;
   }
   const BrickShape s = current_shape( mode, level, false );
   snprintf( buf, buflen, "p1_apply_zmarch_preload_kernel<MODE=%d,NY=%d,LZ=%d,EX_AUX=%d,DEC=0,PFD=%d>", mode, s.ny, s.lz, mode == APPLY_ADD ? 2 : 0, s.pfd );
   return HYTEG_HIP_OK;
}

HYTEG_HIP_API int hyteg_hip_set_apply_shape( int ny, int lz, int pfd )
{
   if ( ny == 0 && lz == 0 && pfd == 0 )
   {
      g_shape_override = BrickShape{ 0, 0, 0 };
      return HYTEG_HIP_OK;
   }
   HH_REQUIRE( shape_compiled( BrickShape{ ny, lz, pfd } ), "set_apply_shape: this brick shape is not compiled in (p1_apply.hip: HYTEG_ZM_SHAPES)" );
   g_shape_override = BrickShape{ ny, lz, pfd };
   return HYTEG_HIP_OK;
}

// host only: the brick table of ( level, ny, lz, xs ) and the store window of every row segment, as the kernel forms them
HYTEG_HIP_API int hyteg_hip_p1_apply_brick_coverage( int level, int ny, int lz, int xs, int dst_phase, unsigned char* count, int* nbricks )
{
   HH_REQUIRE( count && nbricks, "p1_apply_brick_coverage: null pointer" );
   HH_REQUIRE( level >= HYTEG_HIP_MIN_LEVEL && level <= 8, "p1_apply_brick_coverage: level out of range [2,8]" );
   HH_REQUIRE( ny >= 1 && lz >= 1 && lz + 2 <= kBrickMaxSlices && ( xs == 56 || xs == 62 ) && dst_phase >= 0 && dst_phase < 8,
               "p1_apply_brick_coverage: bad shape, x-stride or phase" );
   const int                N = ( 1 << level ) + 1;
   std::vector< BrickTask > tasks;
   build_brick_tasks( level, ny, lz, tasks, xs );
   *nbricks = (int) tasks.size();
   std::fill( count, count + tet64( N ), (unsigned char) 0 );
   for ( const BrickTask& t : tasks )
      for ( int s = 0; s < lz; ++s )
      {
         const int W  = t.W0 - ( s + 1 );
         int       io = t.base[s + 1] + ( W - ( t.y0 - 1 ) ); // (xb, y0, z0 + s)
         for ( int j = 0; j < ny; ++j )
         {
            const int R  = W - ( t.y0 + j );
            int       lo = 1, hi = 1 + std::max( s < t.nz ? std::min( 62, R - 2 - t.xb ) : 0, 0 ); // XS = 62: lanes 1 .. min( 62, R - 2 - xb )
            if ( xs == 56 )
               zm_aligned_window( io, dst_phase, R, t.xb, s < t.nz, lo, hi );
            for ( int l = lo; l < hi; ++l )
            {
               HH_REQUIRE( l <= 62 && io + l >= 0 && io + l < tet64( N ), "p1_apply_brick_coverage: a store window leaves the wave or the array" );
               count[io + l] += 1;
            }
            io += R;
         }
      }
   return HYTEG_HIP_OK;
}

HYTEG_HIP_API int hyteg_hip_set_apply_steps_xs( int xs )
{
   HH_REQUIRE( xs == 0 || xs == 56 || xs == 62, "set_apply_steps_xs: the x-stride is 62 (plain), 56 (aligned store windows) or 0 (default)" );
   g_steps_xs_override = xs;
   return HYTEG_HIP_OK;
}

HYTEG_HIP_API int hyteg_hip_p1_jacobi_cell( double*            dst,
                                            const double*      rhs,
                                            const double*      src,
                                            const double*      invdiag,
                                            int                level,
                                            const double*      w,
                                            double             relax,
                                            hyteg_hip_stream_t stream )
{
   HH_REQUIRE( dst && rhs && src && w, "p1_jacobi_cell: null pointer" );
   HH_REQUIRE( level_ok( level ), "p1_jacobi_cell: level out of range [2,11]" );
   HH_REQUIRE( dst != src, "p1_jacobi_cell: src and dst must not alias" );
   HH_REQUIRE( w[7] != 0.0, "p1_jacobi_cell: zero centre weight" );
   return launch_apply< APPLY_JACOBI >( dst, src, rhs, invdiag, level, w, relax, as_stream( stream ) );
}
}
