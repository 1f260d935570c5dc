// Launch layer of the variable-coefficient P2 operators (kernels_p2_varcoef.hpp).  An operator's .hip file states what is its own in a
// struct L (p2_divkgrad.hip, p2_epsilon.hip):
//    OP                                          its operator policy
//    kInnerMinLevelDefault, kInnerMinLevelEnv    the first level whose inner DoFs the inner form computes, and the variable that overrides it
//    kGatherLanes, kGatherLanesMaxLevel          the lanes per DoF of the gather form, and the last level at which "every DoF" uses them
// The entries take arrays of OP::NC pointers and OP::NC point-class masks.
#pragma once

#include <atomic>
#include <cmath>
#include <cstring>
#include <type_traits>

#include "element_matrices.hpp"
#include "kernels_p2_varcoef.hpp"

namespace {
namespace p2varcoef {

template < class L >
std::atomic< int >& inner_min_level()
{
   static std::atomic< int > v( env_int( L::kInnerMinLevelEnv, L::kInnerMinLevelDefault ) );
   return v;
}
// the body of an operator's set_inner_min_level entry: there is no inner form below level 2
template < class L >
int set_inner_min_level( int level )
{
   const int before = inner_min_level< L >().load();
   inner_min_level< L >().store( level < 2 ? 2 : level );
   return before;
}

template < int NC >
int validate( const std::string& w, double* const* dstV, double* const* dstE, const double* const* srcV, const double* const* srcE, const double* kV,
              const double* kE, int level, const double* geometry, int update )
{
   HH_REQUIRE( dstV && dstE && srcV && srcE && kV && kE && geometry, w + ": null pointer" );
   for ( int j = 0; j < NC; ++j )
      HH_REQUIRE( dstV[j] && dstE[j] && srcV[j] && srcE[j], w + ": null pointer" );
   HH_REQUIRE( level >= 0 && level <= kMaxLevel, w + ": level out of range [0,8]" );
   const std::string alias = w + ": a written array must not alias src, the coefficient or another written array";
   const double*     written[2 * NC];
   for ( int j = 0; j < NC; ++j )
      written[j] = dstV[j], written[NC + j] = dstE[j];
   for ( int a = 0; a < 2 * NC; ++a )
   {
      HH_REQUIRE( written[a] != kV && written[a] != kE, alias );
      for ( int j = 0; j < NC; ++j )
         HH_REQUIRE( written[a] != srcV[j] && written[a] != srcE[j], alias );
      for ( int b = a + 1; b < 2 * NC; ++b )
         HH_REQUIRE( written[a] != written[b], alias );
   }
   HH_REQUIRE( update == HYTEG_HIP_REPLACE || update == HYTEG_HIP_ADD, w + ": bad update type" );
   return HYTEG_HIP_OK;
}

template < class OP >
Args< OP > make_args( double* const* dstV, double* const* dstE, const double* const* srcV, const double* const* srcE, const double* kV, const double* kE,
                      int level, const double* geometry, double alpha, int update, const unsigned* mask, unsigned kinds )
{
   static_assert( sizeof( typename OP::Geometry ) % sizeof( double ) == 0 && std::is_trivially_copyable_v< typename OP::Geometry > );
   Args< OP > A{};
   for ( int j = 0; j < OP::NC; ++j )
      A.dstV[j] = dstV[j], A.dstE[j] = dstE[j], A.srcV[j] = srcV[j], A.srcE[j] = srcE[j], A.mask[j] = mask[j];
   A.kV = kV, A.kE = kE, A.alpha = alpha;
   A.N = ( 1 << level ) + 1, A.update = update, A.kinds = kinds;
   std::memcpy( &A.W, geometry, sizeof( A.W ) ); // the C-ABI's geometry array is the Geometry's numbers in their order
   return A;
}

template < class OP >
unsigned any_mask( const Args< OP >& A )
{
   unsigned any = 0;
   for ( int j = 0; j < OP::NC; ++j )
      any |= A.mask[j];
   return any;
}

// the gather form on the DoFs of A.mask: all entries of the kinds' arrays if a component asks for an inner DoF, else the boundary walk.
// L::kGatherLanes lanes per DoF where the launch is latency-bound (the boundary walk, all DoFs up to L::kGatherLanesMaxLevel, and the
// diagonal, which runs once per operator); one lane per DoF above, where repeating the index decode eight times costs more than the
// round trips (tools/bench_kernels.py --only p2-divkgrad / p2-epsilon)
// E: Plain, or the Epilogue of a fused mode (the kernels that take FusedGatherArgs)
template < class L, bool DIAG = false, class EP = Plain >
int launch_gather( const Args< typename L::OP >& A, int level, hipStream_t s, const EP& E = EP{} )
{
   using OP             = typename L::OP;
   constexpr int  GL    = L::kGatherLanes;
   constexpr bool FUSED = !std::is_same_v< EP, Plain >;
   using GA             = std::conditional_t< FUSED, FusedGatherArgs< OP >, GatherArgs< OP > >;
   GA G;
   G.A = A, G.T = tables();
   if constexpr ( FUSED )
      G.E = E;
   const unsigned all = tet32( (unsigned) A.N ), shell = (unsigned) ( 4 * tri( A.N ) );
   const auto     grid = []( unsigned dofs, int lanes ) { return dim3( ( dofs * lanes + kThreads - 1 ) / kThreads, 8 ); };
   if constexpr ( DIAG )
      hipLaunchKernelGGL( ( gather_kernel< OP, true, GL, true > ), grid( all, GL ), dim3( kThreads ), 0, s, G );
   else if ( !( any_mask( A ) & HYTEG_HIP_MASK_INNER ) )
      hipLaunchKernelGGL( ( gather_kernel< OP, false, GL, false, GA > ), grid( shell, GL ), dim3( kThreads ), 0, s, G );
   else if ( level <= L::kGatherLanesMaxLevel )
      hipLaunchKernelGGL( ( gather_kernel< OP, true, GL, false, GA > ), grid( all, GL ), dim3( kThreads ), 0, s, G );
   else
      hipLaunchKernelGGL( ( gather_kernel< OP, true, 1, false, GA > ), grid( all, 1 ), dim3( kThreads ), 0, s, G );
   HH_CHECK_HIP( hipGetLastError() );
   return HYTEG_HIP_OK;
}

// The shape split of an apply or of a fused mode on the DoFs of A.mask and A.kinds (not all empty).  gather_only: the gather form on
// every DoF; otherwise the gather form on the shell and, from the operator's first inner level, the inner vertex and inner edge launches
template < class L, class EP >
int launch( const Args< typename L::OP >& A, const EP& E, bool gather_only, int level, hipStream_t s )
{
   using OP                 = typename L::OP;
   const unsigned any       = any_mask( A );
   const bool     inner =
       !gather_only && ( any & HYTEG_HIP_MASK_INNER ) && level >= 2 && level >= inner_min_level< L >().load( std::memory_order_relaxed );
   if ( !inner )
      return launch_gather< L, false, EP >( A, level, s, E );
   if ( any & HYTEG_HIP_MASK_SHELL )
   {
      Args< OP > B = A;
      for ( int j = 0; j < OP::NC; ++j )
         B.mask[j] = A.mask[j] & HYTEG_HIP_MASK_SHELL;
      const int rs = launch_gather< L, false, EP >( B, level, s, E );
      if ( rs != HYTEG_HIP_OK )
         return rs;
   }
   const unsigned nb = ( tet32( (unsigned) A.N ) + kThreads - 1 ) / kThreads;
   if constexpr ( std::is_same_v< EP, Plain > )
   {
      if ( A.kinds & 1u )
         hipLaunchKernelGGL( inner_vertex_kernel< OP >, dim3( nb ), dim3( kThreads ), 0, s, A );
      if ( A.kinds & 0xFEu )
         hipLaunchKernelGGL( inner_edge_kernel< OP >, dim3( nb, 7 ), dim3( kThreads ), 0, s, A );
   }
   else
   {
      const FusedArgs< OP > F{ A, E };
      if ( A.kinds & 1u )
         hipLaunchKernelGGL( ( inner_vertex_kernel< OP, FusedArgs< OP > > ), dim3( nb ), dim3( kThreads ), 0, s, F );
      if ( A.kinds & 0xFEu )
         hipLaunchKernelGGL( ( inner_edge_kernel< OP, FusedArgs< OP > > ), dim3( nb, 7 ), dim3( kThreads ), 0, s, F );
   }
   HH_CHECK_HIP( hipGetLastError() );
   return HYTEG_HIP_OK;
}

// dst = alpha A src or dst += alpha A src on the DoFs of the masks and kinds
template < class L >
int apply( const char* who, bool gather_only, double* const* dstV, double* const* dstE, const double* const* srcV, const double* const* srcE,
           const double* kV, const double* kE, const unsigned* mask, int level, const double* geometry, double alpha, int update, unsigned kinds,
           hipStream_t s )
{
   using OP = typename L::OP;
   HH_REQUIRE( mask, std::string( who ) + ": null pointer" );
   const int rc = validate< OP::NC >( who, dstV, dstE, srcV, srcE, kV, kE, level, geometry, update );
   if ( rc != HYTEG_HIP_OK )
      return rc;
   unsigned m[OP::NC], any = 0;
   for ( int j = 0; j < OP::NC; ++j )
      any |= m[j] = mask[j] & HYTEG_HIP_MASK_ALL;
   kinds &= 0xFFu;
   if ( any == 0 || kinds == 0 )
      return HYTEG_HIP_OK;
   return launch< L >( make_args< OP >( dstV, dstE, srcV, srcE, kV, kE, level, geometry, alpha, update, m, kinds ), Plain{}, gather_only, level, s );
}

// ---- the fused modes (kernels_p2_varcoef.hpp, Mode): the arguments of apply plus the mode's operands ----------------------------
// An operand is a pair ( vertex arrays, edge arrays ) of NC pointers each; a pair the mode does not have is { nullptr, nullptr }.
template < class T >
struct Operand
{
   T* const* v;
   T* const* e;
};
// Before any launch: no null pointer among the mode's operands, the level, no written array (dst, t_out, x) equal to another array of
// the call, no array equal to the coefficient.
template < class L >
int fused( const char* who, Mode mode, bool gather_only, Operand< double > dst, Operand< const double > src, Operand< const double > rhs,
           Operand< const double > inv, Operand< double > x, const double* kV, const double* kE, const unsigned* mask, int level,
           const double* geometry, double relax, double cPrev, double cCur, int hasPrev, unsigned kinds, hipStream_t s )
{
   using OP         = typename L::OP;
   constexpr int NC = OP::NC;
   const bool    hasRhs = mode != kChebStep, hasInv = mode != kResidual, hasX = mode == kChebStep;
   const std::string w = who;
   HH_REQUIRE( mask && kV && kE && geometry && dst.v && dst.e && src.v && src.e, w + ": null pointer" );
   HH_REQUIRE( ( !hasRhs || ( rhs.v && rhs.e ) ) && ( !hasInv || ( inv.v && inv.e ) ) && ( !hasX || ( x.v && x.e ) ), w + ": null pointer" );
   const double* written[4 * NC];
   const double* read[6 * NC];
   int           nw = 0, nr = 0;
   for ( int j = 0; j < NC; ++j )
   {
      written[nw++] = dst.v[j], written[nw++] = dst.e[j];
      read[nr++] = src.v[j], read[nr++] = src.e[j];
      if ( hasX )
         written[nw++] = x.v[j], written[nw++] = x.e[j];
      if ( hasRhs )
         read[nr++] = rhs.v[j], read[nr++] = rhs.e[j];
      if ( hasInv )
         read[nr++] = inv.v[j], read[nr++] = inv.e[j];
   }
   for ( int a = 0; a < nw; ++a )
      HH_REQUIRE( written[a], w + ": null pointer" );
   for ( int a = 0; a < nr; ++a )
      HH_REQUIRE( read[a], w + ": null pointer" );
   HH_REQUIRE( level >= 0 && level <= kMaxLevel, w + ": level out of range [0,8]" );
   const std::string alias = w + ": a written array must not alias another array of the call, and no array the coefficient";
   for ( int a = 0; a < nw; ++a )
   {
      HH_REQUIRE( written[a] != kV && written[a] != kE, alias );
      for ( int b = 0; b < nr; ++b )
         HH_REQUIRE( written[a] != read[b], alias );
      for ( int b = a + 1; b < nw; ++b )
         HH_REQUIRE( written[a] != written[b], alias );
   }
   for ( int b = 0; b < nr; ++b )
      HH_REQUIRE( read[b] != kV && read[b] != kE, alias );
   unsigned m[NC], any = 0;
   for ( int j = 0; j < NC; ++j )
      any |= m[j] = mask[j] & HYTEG_HIP_MASK_ALL;
   kinds &= 0xFFu;
   if ( any == 0 || kinds == 0 )
      return HYTEG_HIP_OK;
   Epilogue< OP > E{};
   for ( int j = 0; j < NC; ++j )
   {
      E.rhsV[j] = hasRhs ? rhs.v[j] : nullptr, E.rhsE[j] = hasRhs ? rhs.e[j] : nullptr;
      E.invV[j] = hasInv ? inv.v[j] : nullptr, E.invE[j] = hasInv ? inv.e[j] : nullptr;
      E.xV[j] = hasX ? x.v[j] : nullptr, E.xE[j] = hasX ? x.e[j] : nullptr;
   }
   E.relax = relax, E.cPrev = cPrev, E.cCur = cCur, E.mode = mode, E.hasPrev = hasPrev != 0;
   return launch< L >( make_args< OP >( dst.v, dst.e, src.v, src.e, kV, kE, level, geometry, 1.0, HYTEG_HIP_REPLACE, m, kinds ), E, gather_only, level, s );
}

// dst = rhs - A src
template < class L >
int residual( const char* who, bool gather_only, Operand< double > dst, Operand< const double > src, Operand< const double > rhs, const double* kV,
              const double* kE, const unsigned* mask, int level, const double* geometry, unsigned kinds, hipStream_t s )
{
   return fused< L >( who, kResidual, gather_only, dst, src, rhs, {}, {}, kV, kE, mask, level, geometry, 0.0, 0.0, 0.0, 0, kinds, s );
}
// dst = src + relax invdiag ( rhs - A src )
template < class L >
int jacobi( const char* who, bool gather_only, Operand< double > dst, Operand< const double > src, Operand< const double > rhs,
            Operand< const double > inv, const double* kV, const double* kE, const unsigned* mask, int level, const double* geometry, double relax,
            unsigned kinds, hipStream_t s )
{
   return fused< L >( who, kJacobi, gather_only, dst, src, rhs, inv, {}, kV, kE, mask, level, geometry, relax, 0.0, 0.0, 0, kinds, s );
}
// t_out = invdiag ( rhs - A x ); x is not updated
template < class L >
int chebyshev_start( const char* who, bool gather_only, Operand< double > tOut, Operand< const double > x, Operand< const double > rhs,
                     Operand< const double > inv, const double* kV, const double* kE, const unsigned* mask, int level, const double* geometry,
                     unsigned kinds, hipStream_t s )
{
   return fused< L >( who, kChebStart, gather_only, tOut, x, rhs, inv, {}, kV, kE, mask, level, geometry, 0.0, 0.0, 0.0, 0, kinds, s );
}
// t_out = invdiag A t_in; x = ( x + c_prev t_in ) + c_cur t_out, the first summand only if has_prev
template < class L >
int chebyshev_step( const char* who, bool gather_only, Operand< double > tOut, Operand< double > x, Operand< const double > tIn,
                    Operand< const double > inv, const double* kV, const double* kE, const unsigned* mask, int level, const double* geometry,
                    double cPrev, double cCur, int hasPrev, unsigned kinds, hipStream_t s )
{
   return fused< L >( who, kChebStep, gather_only, tOut, tIn, {}, inv, x, kV, kE, mask, level, geometry, 0.0, cPrev, cCur, hasPrev, kinds, s );
}

// every DoF of the NC diag arrays receives the diagonal entry of its component's diagonal block
template < class L >
int diagonal( const char* who, double* const* diagV, double* const* diagE, const double* kV, const double* kE, int level, const double* geometry,
              hipStream_t s )
{
   using OP = typename L::OP;
   HH_REQUIRE( diagV && diagE && kV && kE, std::string( who ) + ": null pointer" );
   const double* srcV[OP::NC]; // never read
   const double* srcE[OP::NC];
   unsigned      all[OP::NC];
   for ( int j = 0; j < OP::NC; ++j )
      srcV[j] = kV, srcE[j] = kE, all[j] = HYTEG_HIP_MASK_ALL;
   const int rc = validate< OP::NC >( who, diagV, diagE, srcV, srcE, kV, kE, level, geometry, HYTEG_HIP_REPLACE );
   if ( rc != HYTEG_HIP_OK )
      return rc;
   return launch_gather< L, true >( make_args< OP >( diagV, diagE, srcV, srcE, kV, kE, level, geometry, 1.0, HYTEG_HIP_REPLACE, all, 0xFFu ), level, s );
}

// The front of an operator's geometry entry: per micro-cell type t the volume V and the gradients g_a of the barycentric functions of
// a micro-cell of that type, handed to pack( t, V, g ), which writes the operator's numbers.
template < class Pack >
int geometry( const char* who, const double* macro_vertex_coords, int level, const double* out, Pack pack )
{
   HH_REQUIRE( macro_vertex_coords && out, std::string( who ) + ": null pointer" );
   HH_REQUIRE( level >= 0 && level <= kMaxLevel, std::string( who ) + ": level out of range [0,8]" );
   double cc[4][3];
   for ( int v = 0; v < 4; ++v )
      for ( int r = 0; r < 3; ++r )
         cc[v][r] = macro_vertex_coords[3 * v + r];
   for ( int t = 0; t < 6; ++t )
   {
      double c[4][3], g[4][3];
      elmat::micro_cell_coords( cc, int64_t( 1 ) << level, t, c );
      const double V = elmat::gradients( c, g );
      HH_REQUIRE( V > 0.0 && std::isfinite( V ), std::string( who ) + ": degenerate macro-cell" );
      pack( t, V, g );
   }
   return HYTEG_HIP_OK;
}

} // namespace p2varcoef
} // namespace
