// Kernels of the variable-coefficient P2 operators on one macro-cell: a P2 coefficient k, the integrand of degree 4 on a micro-cell
// integrated exactly.  An operator of the family is a policy struct OP (kernels_p2_divkgrad.hpp, kernels_p2_epsilon.hpp):
//    NC                                               the number of components of src and dst: 1 or 3 (the coefficient is one more P2 array)
//    Geometry                                         its numbers per ( macro-cell, level ), passed in the kernel arguments
//    element_rows( W, t, coef, u, row, res )          row `row` of the NC components of A_e u on a micro-cell of type t, without alpha
//    index( at )                                      the form in which the inner kernels index their loads (see there)
// element_rows takes the Geometry and the type; handed a pointer to the type's numbers instead, every kernel compiles to the same
// instructions (profiles/p2_varcoef_checks.txt), so the call that needs no accessor stays.  Its row selection is written out in each
// policy: as a function of out[10] it becomes an indexed read of an array that the compiler places in LDS.
// What the element matrices share -- the moments of the coefficient and the weights of grad u -- is below, in the notation of
// kernels_p2_divkgrad.hpp.
//
// Two forms.  gather_kernel: the sibling of p2_elementwise_kernel (kernels_p2_gather.hpp), a lane group per DoF, the adjacent micro-cells
// from P2Tables with the inside test: every level's boundary DoFs, all DoFs of levels 0-1, the diagonal, and -- through an entry of its
// own -- every DoF (the second implementation).  inner_vertex_kernel / inner_edge_kernel: the inner DoFs from level 2, the destination
// kind a template parameter and the adjacent micro-cells (24 of a vertex DoF, 4-6 of an edge DoF) with the offsets of their ten DoFs a
// compile-time list, so a thread is straight-line code whose lanes run along x.  Both add the micro-cells' contributions in a fixed
// order; no atomics, no LDS, no scratch.  Every component has a point-class mask of its own: a component whose mask excludes a DoF is
// computed but not stored.  32-bit indices: levels 0 .. kMaxLevel.
//
// Fused modes.  At its store a thread (or the first lane of a group) holds the complete ( A src )_j of its DoF.  The kernels whose
// arguments carry an Epilogue replace the plain store by one of four epilogues, selected by a wave-uniform run-time mode, so that each
// form is compiled once more and not four times (`epilogue` below).  rhs, invdiag and x are read at the DoF's own index only.
#pragma once

#include "kernels_p2_gather.hpp"

namespace {
namespace p2varcoef {

constexpr int kMaxLevel = 8; // 6 tet( 256 ) + tet( 255 ) entries: far below 2^31

template < class OP >
struct Args
{
   static constexpr int  NC = OP::NC;
   double*               dstV[NC];
   double*               dstE[NC];
   const double*         srcV[NC];
   const double*         srcE[NC];
   const double*         kV;
   const double*         kE;
   double                alpha;
   int                   N, update;
   unsigned              mask[NC], kinds;
   typename OP::Geometry W;
};
template < class OP >
struct GatherArgs
{
   Args< OP > A;
   P2Tables   T;
};

// what replaces the store of ( A src )_j (alpha = 1, Replace); dst, src: the arrays of Args
//    kResidual    dst = rhs - A src
//    kJacobi      dst = src + relax invdiag ( rhs - A src )              smooth_jac's four statements in their order; the compiler may
//                 contract the last multiply-add (here and in kChebStep) into one FMA, which the composed passes do not
//    kChebStart   dst = invdiag ( rhs - A src )                          src is x, which is not updated here
//    kChebStep    dst = invdiag A src;  x = ( x + cPrev src ) + cCur dst, the first summand only if hasPrev (src is t_in, dst t_out;
//                 x is read and written at the DoF's own index by the thread that owns it: it is not a source of the operator)
enum Mode : int
{
   kResidual  = 0,
   kJacobi    = 1,
   kChebStart = 2,
   kChebStep  = 3
};
struct Plain
{};
template < class OP >
struct Epilogue
{
   static constexpr int NC = OP::NC;
   const double*        rhsV[NC]; // null where the mode does not read them
   const double*        rhsE[NC];
   const double*        invV[NC];
   const double*        invE[NC];
   double*              xV[NC];
   double*              xE[NC];
   double               relax, cPrev, cCur;
   int                  mode, hasPrev;
};
// the arguments of the fused kernels: those of the plain kernels first, at their offsets
template < class OP >
struct FusedArgs
{
   Args< OP >     A;
   Epilogue< OP > E;
};
template < class OP >
struct FusedGatherArgs
{
   Args< OP >     A;
   P2Tables       T;
   Epilogue< OP > E;
};
template < class OP >
__device__ __forceinline__ const Args< OP >& args_of( const Args< OP >& K )
{
   return K;
}
template < class OP >
__device__ __forceinline__ const Args< OP >& args_of( const FusedArgs< OP >& K )
{
   return K.A;
}
template < class OP >
__device__ __forceinline__ Plain epilogue_of( const Args< OP >& )
{
   return Plain{};
}
template < class OP >
__device__ __forceinline__ const Epilogue< OP >& epilogue_of( const FusedArgs< OP >& K )
{
   return K.E;
}

// component j of the DoF at entry `at` of the vertex array or of the edge array: v = ( A src )_j, complete.  Every branch is
// wave-uniform.  Both store streams of kChebStep are behind the caller's mask test.
template < class OP >
__device__ __forceinline__ void epilogue( const Args< OP >& A, const Epilogue< OP >& E, bool vertex, int j, int at, double v )
{
   double* out = ( vertex ? A.dstV[j] : A.dstE[j] ) + at;
   if ( E.mode == kResidual )
   {
      *out = ( vertex ? E.rhsV[j] : E.rhsE[j] )[at] - v;
      return;
   }
   const double inv = ( vertex ? E.invV[j] : E.invE[j] )[at];
   if ( E.mode == kChebStep )
   {
      double*      x = ( vertex ? E.xV[j] : E.xE[j] ) + at;
      const double t = inv * v;
      const double p = E.hasPrev ? *x + E.cPrev * ( vertex ? A.srcV[j] : A.srcE[j] )[at] : *x;
      *out           = t;
      *x             = p + E.cCur * t;
      return;
   }
   const double d = inv * ( ( vertex ? E.rhsV[j] : E.rhsE[j] )[at] - v );
   *out           = E.mode == kJacobi ? ( vertex ? A.srcV[j] : A.srcE[j] )[at] + E.relax * d : d;
}

constexpr int kLocal[4][4] = { { 0, 9, 8, 7 }, { 9, 1, 6, 5 }, { 8, 6, 2, 4 }, { 7, 5, 4, 3 } }; // fenics::P2DoFMap

// 840 Q_cd / |e| from the ten coefficient values of a micro-cell
__device__ __forceinline__ void moments( const double ( &k )[10], double ( &Q )[4][4] )
{
   double K[4][4], r[4];
#pragma unroll
   for ( int a = 0; a < 4; ++a )
   {
      K[a][a] = k[a];
#pragma unroll
      for ( int b = a + 1; b < 4; ++b )
         K[a][b] = K[b][a] = 2.0 * k[kLocal[a][b]] - 0.5 * ( k[a] + k[b] );
   }
   double s = 0.0, tr = 0.0;
#pragma unroll
   for ( int a = 0; a < 4; ++a )
   {
      r[a] = ( K[a][0] + K[a][1] ) + ( K[a][2] + K[a][3] );
      s += r[a];
      tr += K[a][a];
   }
   const double st = s + tr;
#pragma unroll
   for ( int c = 0; c < 4; ++c )
   {
      Q[c][c] = 2.0 * st + 8.0 * r[c] + 12.0 * K[c][c];
#pragma unroll
      for ( int d = c + 1; d < 4; ++d )
         Q[c][d] = Q[d][c] = st + 2.0 * ( r[c] + r[d] ) + 2.0 * ( K[c][d] + ( K[c][c] + K[d][d] ) );
   }
}
// grad u = sum_b ( sum_d w_bd l_d ) g_b from the ten values of u
__device__ __forceinline__ void weights( const double ( &u )[10], double ( &w )[4][4] )
{
#pragma unroll
   for ( int b = 0; b < 4; ++b )
#pragma unroll
      for ( int d = 0; d < 4; ++d )
         w[b][d] = b == d ? 3.0 * u[b] : 4.0 * u[kLocal[b][d]] - u[b];
}
__device__ inline int block_start( int n, int kind ) { return ( kind - 1 ) * (int) tet32( (unsigned) n ); }

// ---- gather form: a group of G lanes per DoF, micro-cells from the tables ------------------------------------------------------
// ALL: group q is entry q of the kind's array; otherwise the boundary DoFs only (p2_decode_boundary).
// DIAG: component i of every DoF receives the sum of A_e^{ii}[row][row] (src is not read): the row function on the unit vector of
// the DoF in component i alone, once per component.
// KA = FusedGatherArgs< OP >: the epilogue of GA.E.mode in place of the store.
template < class OP, bool ALL, int G, bool DIAG, class KA = GatherArgs< OP > >
__global__ __launch_bounds__( kThreads ) void gather_kernel( const KA GA )
{
   constexpr int  NC    = OP::NC;
   constexpr bool FUSED = !std::is_same_v< KA, GatherArgs< OP > >;
   static_assert( !( FUSED && DIAG ), "the diagonal has no fused mode" );
   const Args< OP >& A  = GA.A;
   const int         c  = blockIdx.y; // destination kind
   const int         N = A.N, n = N - 1;
   const int         W = c == 0 ? N : ( c == 7 ? n - 1 : n );
   if ( W <= 0 || !( ( A.kinds >> c ) & 1u ) )
      return;
   const int lane = threadIdx.x & ( G - 1 );
   const int q    = blockIdx.x * ( kThreads / G ) + (int) threadIdx.x / G;
   int       x, y, z;
   if ( !( ALL ? p2_decode_all( W, q, x, y, z ) : p2_decode_boundary( W, q, x, y, z ) ) )
      return;
   const int cls = c == 0 ? slot_from_flags< 14 >( z == 0, y == 0, x == 0, x + y + z == N - 1 ) : edge_class( N, x, y, z, c - 1 );
   unsigned  any = A.mask[0];
#pragma unroll
   for ( int j = 1; j < NC; ++j )
      any |= A.mask[j];
   if ( !( ( any >> cls ) & 1u ) )
      return;
   // every lane of a DoF's group is still here, or none is
   const int i = cell_index( W, x, y, z );
   // one adjacent micro-cell: alpha * ( the NC rows of its element matrix ) . ( its 10 NC source values )
   auto contribution = [&]( int l, double( &part )[NC] ) -> bool {
      const Entry en = GA.T.entries[c][l];
      const int   t = en.type, mx = x - en.ox, my = y - en.oy, mz = z - en.oz;
      const int   rows = n - kRowDeficit[t];
      if ( mx < 0 || my < 0 || mz < 0 || mx + my + mz > rows - 1 )
         return false; // the micro-cell is not inside the macro-cell; inside, all its ten DoFs are
      double k[10], u[NC][10];
#pragma unroll
      for ( int d = 0; d < 10; ++d )
      {
         const LocalDof ld = GA.T.local[t][d];
         const int      px = mx + ld.ox, py = my + ld.oy, pz = mz + ld.oz;
         const int      at = ld.kind == 0 ? cell_index( N, px, py, pz ) : block_start( n, ld.kind ) + cell_index( ld.kind == 7 ? n - 1 : n, px, py, pz );
         k[d]              = ld.kind == 0 ? A.kV[at] : A.kE[at];
         if constexpr ( !DIAG )
         {
#pragma unroll
            for ( int j = 0; j < NC; ++j )
               u[j][d] = ld.kind == 0 ? A.srcV[j][at] : A.srcE[j][at];
         }
      }
      if constexpr ( DIAG )
      {
#pragma unroll 1
         for ( int m = 0; m < NC; ++m )
         {
#pragma unroll
            for ( int j = 0; j < NC; ++j )
#pragma unroll
               for ( int d = 0; d < 10; ++d )
                  u[j][d] = ( j == m && d == en.row ) ? 1.0 : 0.0;
            double o[NC];
            OP::element_rows( A.W, t, k, u, en.row, o );
#pragma unroll
            for ( int j = 0; j < NC; ++j )
               part[j] = m == j ? o[j] : part[j];
         }
      }
      else
      {
         double o[NC];
         OP::element_rows( A.W, t, k, u, en.row, o );
#pragma unroll
         for ( int j = 0; j < NC; ++j )
            part[j] = A.alpha * o[j];
      }
      return true;
   };
   double acc[NC] = {};
   if constexpr ( G > 1 )
   {
      constexpr int      kSlots = 24 / G;
      double             part[kSlots][NC];
      unsigned long long vmask[kSlots];
#pragma unroll
      for ( int k = 0; k < kSlots; ++k )
      {
#pragma unroll
         for ( int j = 0; j < NC; ++j )
            part[k][j] = 0.0;
         const int  l     = lane + k * G;
         const bool valid = l < GA.T.nentries[c] && contribution( l, part[k] );
         vmask[k]         = __ballot( valid );
      }
      p2_group_sum< G, NC >( part, vmask, acc );
      if ( lane != 0 )
         return;
   }
   else
   {
      static_assert( !DIAG, "the diagonal reads part before it writes it: only with lane groups, which zero it" );
      for ( int l = 0; l < GA.T.nentries[c]; ++l )
      {
         double part[NC];
         if ( contribution( l, part ) )
         {
#pragma unroll
            for ( int j = 0; j < NC; ++j )
               acc[j] += part[j];
         }
      }
   }
   const int at = c == 0 ? i : block_start( n, c ) + i;
#pragma unroll
   for ( int j = 0; j < NC; ++j )
   {
      if ( !( ( A.mask[j] >> cls ) & 1u ) )
         continue;
      if constexpr ( FUSED )
         epilogue( A, GA.E, c == 0, j, at, acc[j] );
      else
      {
         double* out = ( c == 0 ? A.dstV[j] : A.dstE[j] ) + at;
         *out        = A.update == HYTEG_HIP_ADD ? *out + acc[j] : acc[j];
      }
   }
}

// ---- inner form: destination kind C, compile-time micro-cell list -------------------------------------------------------------
struct CellList
{
   int n;
   int type[24], row[24], ox[24], oy[24], oz[24];
};
// the micro-cells ( type, base = dof - offset ) that hold a DoF of kind c as their local DoF `row`, in the order ( type, row )
constexpr CellList cells( int c )
{
   CellList L{};
   for ( int t = 0; t < 6; ++t )
      for ( int k = 0; k < 10; ++k )
      {
         const CLocal l = c_local( t, k );
         if ( l.kind != c )
            continue;
         L.type[L.n] = t, L.row[L.n] = k, L.ox[L.n] = l.ox, L.oy[L.n] = l.oy, L.oz[L.n] = l.oz;
         ++L.n;
      }
   return L;
}
template < int C >
struct CellsOf
{
   static constexpr CellList value = cells( C );
};
template < int T, int D >
struct LocalOf
{
   static constexpr CLocal value = c_local( T, D );
};

// a DoF is inner if no face of the macro-cell holds all its end points
template < int C >
__device__ __forceinline__ bool is_inner( int N, int x, int y, int z )
{
   if constexpr ( C == 0 )
      return x > 0 && y > 0 && z > 0 && x + y + z < N - 1;
   else
   {
      constexpr int ax = kEdgeEndsHost[C - 1][0][0], ay = kEdgeEndsHost[C - 1][0][1], az = kEdgeEndsHost[C - 1][0][2];
      constexpr int bx = kEdgeEndsHost[C - 1][1][0], by = kEdgeEndsHost[C - 1][1][1], bz = kEdgeEndsHost[C - 1][1][2];
      const bool    f0 = z + az == 0 && z + bz == 0, f1 = y + ay == 0 && y + by == 0, f2 = x + ax == 0 && x + bx == 0;
      const bool    f3 = x + y + z + ( ax + ay + az ) == N - 1 && x + y + z + ( bx + by + bz ) == N - 1;
      return !( f0 || f1 || f2 || f3 );
   }
}

// Index arithmetic of the inner form.  Every value a thread reads sits at a compile-time offset ( DX, DY, DZ ) from the thread's own
// logical index ( x, y, z ) in an array of width N ( vertex DoFs ), n ( edge DoFs X .. YZ ) or n - 1 ( XYZ ).  The index of ( x, y, z )
// itself is formed once per width; with Wz = width - z the layout  index = tet( W ) - tet( Wz ) + y Wz - y ( y - 1 ) / 2 + x  gives
//    index( x + DX, y + DY, z + DZ ) - index( x, y, z ) = DX + tet( Wz ) - tet( Wz - DZ ) + DY ( Wz - y ) - DZ y - DY DZ - ( DY^2 - DY ) / 2,
// a polynomial identity (the base index need not be a valid entry).  Per load that is a handful of 32-bit operations, shared where
// ( DY, DZ ) repeat.
struct Base
{
   int b[3], wz[3]; // by width: 0: N, 1: n, 2: n - 1
   int y, te;       // te = tet( n ): length of an edge block
};
__device__ __forceinline__ int tet_of( int w ) { return ( w * ( w + 1 ) * ( w + 2 ) ) / 6; }
__device__ __forceinline__ Base base_of( int N, int x, int y, int z )
{
   Base B;
#pragma unroll
   for ( int s = 0; s < 3; ++s )
   {
      const int W = N - s, wz = W - z;
      B.wz[s]     = wz;
      B.b[s]      = tet_of( W ) - tet_of( wz ) + y * wz - ( y * ( y - 1 ) ) / 2 + x;
   }
   B.y = y, B.te = tet_of( N - 1 );
   return B;
}
template < int K, int DX, int DY, int DZ >
__device__ __forceinline__ int index_at( const Base& B )
{
   static_assert( DZ >= -2 && DZ <= 2, "offsets of the DoFs of a micro-cell" );
   constexpr int S  = K == 0 ? 0 : ( K == 7 ? 2 : 1 );
   const int     wz = B.wz[S], y = B.y;
   int           sl = 0;
   if constexpr ( DZ == 1 )
      sl = tri( wz );
   else if constexpr ( DZ == -1 )
      sl = -tri( wz + 1 );
   else if constexpr ( DZ == 2 )
      sl = tri( wz ) + tri( wz - 1 );
   else if constexpr ( DZ == -2 )
      sl = -tri( wz + 1 ) - tri( wz + 2 );
   const int at = B.b[S] + DX + sl + DY * ( wz - y ) - DZ * y - DY * DZ - ( DY * DY - DY ) / 2;
   return K == 0 ? at : ( K - 1 ) * B.te + at;
}

// micro-cell I of the list of kind C.  The loads are indexed by OP::index( at ): a sign-extended index makes every ( array, offset )
// pair a 64-bit lane address of its own; as the unsigned 28-bit number it is (the arrays of level 8 have fewer than 2^25 entries) the
// byte offset provably fits 32 bits, so a load is  scalar base pointer + 32-bit lane offset  and the offset register of a DoF serves
// every field (profiles/p2_epsilon.txt).  Each operator keeps the form it was measured with.
template < class OP, int C, int I >
__device__ __forceinline__ void inner_cell( const Args< OP >& A, const Base& B, double ( &acc )[OP::NC] )
{
   constexpr int NC = OP::NC;
   constexpr int T = CellsOf< C >::value.type[I], ROW = CellsOf< C >::value.row[I];
   constexpr int MX = -CellsOf< C >::value.ox[I], MY = -CellsOf< C >::value.oy[I], MZ = -CellsOf< C >::value.oz[I];
   double        k[10], u[NC][10];
   [&]< int... D >( std::integer_sequence< int, D... > ) {
      const decltype( OP::index( 0 ) ) at[10] = { OP::index(
          index_at< LocalOf< T, D >::value.kind, MX + LocalOf< T, D >::value.ox, MY + LocalOf< T, D >::value.oy, MZ + LocalOf< T, D >::value.oz >( B ) )... };
      ( ( k[D] = ( LocalOf< T, D >::value.kind == 0 ? A.kV : A.kE )[at[D]] ), ... );
#pragma unroll
      for ( int j = 0; j < NC; ++j )
         ( ( u[j][D] = ( LocalOf< T, D >::value.kind == 0 ? A.srcV[j] : A.srcE[j] )[at[D]] ), ... );
   }
   ( std::make_integer_sequence< int, 10 >{} );
   double o[NC];
   OP::element_rows( A.W, T, k, u, ROW, o );
#pragma unroll
   for ( int j = 0; j < NC; ++j )
      acc[j] += A.alpha * o[j];
   // one micro-cell at a time: the 24 cells of a vertex DoF read 240 ( NC + 1 ) values, which must not all be in flight at once
   __builtin_amdgcn_sched_barrier( 0 );
}

template < class OP, int C, class EP >
__device__ __forceinline__ void inner_body( const Args< OP >& A, const EP& E )
{
   constexpr int NC     = OP::NC;
   constexpr int NCELLS = CellsOf< C >::value.n; // forced constant evaluation: none of the table code may run on the device
   static_assert( NC == 1 || NC == 3, "the register pin below is written out for three components" );
   const int N = A.N, n = N - 1;
   const int W = C == 0 ? N : ( C == 7 ? n - 1 : n );
   const int q = blockIdx.x * kThreads + (int) threadIdx.x;
   if ( W <= 0 || q >= tet_of( W ) )
      return;
   const int z = slice_of( W, q );
   const int j = q - ( tet_of( W ) - tet_of( W - z ) );
   const int y = row_of( W - z, j );
   const int x = j - row_start( W - z, y );
   if ( !is_inner< C >( N, x, y, z ) )
      return;
   const Base B       = base_of( N, x, y, z );
   double     acc[NC] = {};
   [&]< int... I >( std::integer_sequence< int, I... > ) { ( inner_cell< OP, C, I >( A, B, acc ), ... ); }
   ( std::make_integer_sequence< int, NCELLS >{} );
   // The sums are complete HERE.  Without a use in this block the compiler sinks each component's half of the arithmetic (E, S and the
   // running sum of every cell) into that component's conditional store below and keeps the Z of all cells alive until then: 10 KB of
   // scratch per lane in the epsilon vertex kernel (profiles/p2_epsilon.txt).
   if constexpr ( NC == 3 )
      asm volatile( "" : "+v"( acc[0] ), "+v"( acc[1] ), "+v"( acc[2] ) );
   const int at = C == 0 ? q : ( C - 1 ) * B.te + q;
#pragma unroll
   for ( int k = 0; k < NC; ++k )
   {
      if constexpr ( NC > 1 ) // one component: the launch layer starts this kernel only for a mask with the inner class
         if ( !( ( A.mask[k] >> 14 ) & 1u ) ) // inner DoFs are point class 14
            continue;
      if constexpr ( !std::is_same_v< EP, Plain > )
         epilogue( A, E, C == 0, k, at, acc[k] );
      else
      {
         double* out = ( C == 0 ? A.dstV[k] : A.dstE[k] ) + at;
         *out        = A.update == HYTEG_HIP_ADD ? *out + acc[k] : acc[k];
      }
   }
}

// the inner vertex DoFs (24 micro-cells each, the most registers) and, blockIdx.y + 1 = destination kind, the inner edge DoFs of the
// kinds of A.kinds: two launches, so that the edge kinds are not held to the vertex kind's occupancy.  KA = FusedArgs< OP >: the
// epilogue of K.E.mode in place of the store
template < class OP, class KA = Args< OP > >
__global__ __launch_bounds__( kThreads ) void inner_vertex_kernel( const KA K )
{
   inner_body< OP, 0 >( args_of< OP >( K ), epilogue_of< OP >( K ) );
}
template < class OP, class KA = Args< OP > >
__global__ __launch_bounds__( kThreads ) void inner_edge_kernel( const KA K )
{
   const Args< OP >& A = args_of< OP >( K );
   const int         c = blockIdx.y + 1;
   if ( !( ( A.kinds >> c ) & 1u ) )
      return;
   [&]< int... C >( std::integer_sequence< int, C... > ) { ( ( c == C + 1 ? inner_body< OP, C + 1 >( A, epilogue_of< OP >( K ) ) : void() ), ... ); }
   ( std::make_integer_sequence< int, 7 >{} );
}

} // namespace p2varcoef
} // namespace
