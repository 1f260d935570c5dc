// Kernels of the variable-coefficient P1 operators on one macro-cell: the element matrix of a micro-cell e is the mean of a P1
// coefficient over the 4 vertices of e times a constant matrix of the micro-cell's type, with zero row sums.  The value at a point p
// is then a sum over the micro-cells at p of  coefficient sum( e ) * ( weights of e's type applied to the differences u_j - u_p ).
// An operator of the family is a policy struct OP (kernels_divkgrad.hpp, kernels_epsilon.hpp):
//    NC                                        the number of components of src and dst (the coefficient is one more array)
//    Weights                                   its wave-uniform weights, passed in the kernel arguments
//    cell_term< C >( A, d, k, acc )            inner points: adds the adjacent micro-cell C's contribution to acc[NC], weights A.W
//    point_cell< DIAG >( A, t, i, m, d, acc )  point form: the same for one micro-cell known to lie inside the macro-cell
// Both take the kernel's Args A and read A.W only.  Handing them A.W instead moves the first cell's weight loads in the compiled
// epsilon z-march and with them the register allocation of eight of its nine instantiations (2 x 4 bricks, Replace: 6 AGPRs more).
// Two kinds of kernel:
//  * zmarch_kernel: the inner points (24 micro-cells each), a register z-march in the manner of kernels_apply_zmarch.hpp.  A wave
//    owns a brick of NY rows x 64 x-positions x LZ slices, loads every row segment of the NC sources AND of the coefficient once
//    through buffer loads with wave-uniform bases, keeps the live slices of all of them in registers and stores dst nontemporally.
//    Modes (enum Mode): Replace, Add, the fused Jacobi step, and the fused steps of a multigrid cycle -- the residual and the two
//    kinds of Chebyshev step, the second with x as a second store stream.
//    The x-1 / x+1 neighbours are DPP wave shifts of the loaded rows themselves: coefficient * K * u is not linear in a partial sum
//    that could be shifted instead, as the constant-stencil kernel does.
//  * shell_kernel / inner_point_kernel: one thread per point, testing which of the point's 24 micro-cells lie inside the macro-cell
//    (the shell classes, levels 0 and 1, the diagonals; over the inner points it is the form the z-march is measured against).
#pragma once

#include "element_matrices.hpp"
#include "kernels_apply_zmarch.hpp"
#include "shell.hpp"

namespace hyteg_hip {
namespace varcoef {

// vertex pairs of a micro-cell in the order (0,1) (0,2) (0,3) (1,2) (1,3) (2,3)
constexpr int pair_index( int a, int b )
{
   const int lo = a < b ? a : b, hi = a < b ? b : a;
   return lo == 0 ? hi - 1 : ( lo == 1 ? hi + 1 : 5 );
}
constexpr int micro_vert( int t, int k, int r )
{
   constexpr int V[6][4][3] = { { { 0, 0, 0 }, { 1, 0, 0 }, { 0, 1, 0 }, { 0, 0, 1 } }, { { 1, 0, 0 }, { 1, 1, 0 }, { 0, 1, 0 }, { 1, 0, 1 } },
                                { { 1, 0, 0 }, { 0, 1, 0 }, { 1, 0, 1 }, { 0, 0, 1 } }, { { 1, 1, 0 }, { 1, 1, 1 }, { 0, 1, 1 }, { 1, 0, 1 } },
                                { { 1, 0, 1 }, { 0, 1, 1 }, { 0, 0, 1 }, { 0, 1, 0 } }, { { 0, 1, 0 }, { 1, 1, 0 }, { 1, 0, 1 }, { 0, 1, 1 } } };
   return V[t][k][r]; // = elmat::kMicroCellVerts, usable in constant expressions on the device
}
// index in the 15 stencil directions (C-ABI weight order) of the edge from local vertex i to local vertex j of a type-t micro-cell
constexpr int edge_dir( int t, int i, int j )
{
   const int dx = micro_vert( t, j, 0 ) - micro_vert( t, i, 0 ), dy = micro_vert( t, j, 1 ) - micro_vert( t, i, 1 ),
             dz = micro_vert( t, j, 2 ) - micro_vert( t, i, 2 );
   for ( int k = 0; k < 15; ++k )
      if ( kStencilOffsC[k][0] == dx && kStencilOffsC[k][1] == dy && kStencilOffsC[k][2] == dz )
         return k;
   return -1;
}

// Adjacent micro-cell C = 4 t + i of an inner point: the type-t micro-cell that has the point as its local vertex i.  ja, jb, jc are
// its other vertices and a, b, c the stencil directions from the point to them.
template < int C >
struct Cell
{
   static constexpr int t = C / 4, i = C % 4;
   static constexpr int ja = ( i + 1 ) % 4, jb = ( i + 2 ) % 4, jc = ( i + 3 ) % 4;
   static constexpr int a = edge_dir( t, i, ja ), b = edge_dir( t, i, jb ), c = edge_dir( t, i, jc );
   static_assert( a >= 0 && b >= 0 && c >= 0 && a != 7 && b != 7 && c != 7, "every micro-cell edge is a stencil direction" );
   // the coefficient at the cell's four vertices, summed; k[15]: the coefficient at the stencil neighbours (index 7: the point itself)
   __device__ static double coef_sum( const double ( &k )[15] ) { return ( k[7] + k[a] ) + ( k[b] + k[c] ); }
};

enum Mode
{
   REPLACE = 0,
   ADD     = 1,
   JACOBI  = 2, // dst_i = src_i + omega * invdiag_i * ( rhs_i - ( A src )_i )
   DIAG    = 3, // dst_i += diagonal of A^{ii} (point kernels only; src unused)
   // the fused steps of a multigrid residual and of a Chebyshev smoother (inner points only; the shell is composed by the host layer)
   RESIDUAL   = 4, // dst_i = rhs_i - ( A src )_i
   CHEB_START = 5, // dst_i = invdiag_i * ( rhs_i - ( A src )_i )
   CHEB_STEP  = 6  // dst_i = invdiag_i * ( A src )_i,  x_i = ( x_i + cPrev * src_i ) + cCur * dst_i  (first summand only if hasPrev);
                   // src is t_in and dst is t_out.  x is no stencil source: read and rewritten at the output points only, as Add reads dst
};
constexpr bool reads_rhs( int m ) { return m == JACOBI || m == RESIDUAL || m == CHEB_START; }
constexpr bool reads_invdiag( int m ) { return m == JACOBI || m == CHEB_START || m == CHEB_STEP; }

template < class OP >
struct Args
{
   static constexpr int NC = OP::NC;
   double*              dst[NC];
   const double*        src[NC];
   const double*        coef;
   const double*        rhs[NC];     // JACOBI, RESIDUAL, CHEB_START
   const double*        invdiag[NC]; // JACOBI, CHEB_START, CHEB_STEP
   unsigned             bytes;       // size of a cell array in bytes (buffer range)
   int                  N;           // 2^level + 1
   unsigned             comps;       // z-march / inner point kernel: bit i = destination component i is written.  Tested where
                                     // NC > 1: launch_inner launches nothing when no component is written
   unsigned             masks[NC];   // shell kernel: the class mask of each destination component
   double               omega;
   typename OP::Weights W;
   // CHEB_STEP (behind W: the kernel argument offsets of the other modes stay where they were)
   double* x[NC];
   double  cPrev, cCur;
   int     hasPrev;
};

// the 15 stencil values of one marched array around slice Q, row j + 1, in the C-ABI's direction order (kStencilOffsC);
// rows: j = y - 1, j + 1 = y, j + 2 = y + 1
template < int Q, int SLICES, int ROWS >
__device__ inline void gather( const double ( &P )[SLICES][ROWS], int j, double ( &v )[15] )
{
   v[0]  = P[Q - 1][j + 1];
   v[1]  = zm_lane_plus_1( P[Q - 1][j + 1] );
   v[2]  = zm_lane_minus_1( P[Q - 1][j + 2] );
   v[3]  = P[Q - 1][j + 2];
   v[4]  = P[Q][j];
   v[5]  = zm_lane_plus_1( P[Q][j] );
   v[6]  = zm_lane_minus_1( P[Q][j + 1] );
   v[7]  = P[Q][j + 1];
   v[8]  = zm_lane_plus_1( P[Q][j + 1] );
   v[9]  = zm_lane_minus_1( P[Q][j + 2] );
   v[10] = P[Q][j + 2];
   v[11] = P[Q + 1][j];
   v[12] = zm_lane_plus_1( P[Q + 1][j] );
   v[13] = zm_lane_minus_1( P[Q + 1][j + 1] );
   v[14] = P[Q + 1][j + 1];
}

// the sum over the 24 micro-cells at an inner point.  d[c][15]: the differences u_j - u_p of component c to the point's stencil
// neighbours, k[15]: the coefficient there (index 7: the point itself)
template < class OP, int... Cs >
__device__ inline void inner_sum( const Args< OP >& A, const double ( &d )[OP::NC][15], const double ( &k )[15], double ( &acc )[OP::NC],
                                  std::integer_sequence< int, Cs... > )
{
   ( OP::template cell_term< Cs >( A, d, k, acc ), ... );
}

template < class OP, int MODE, int NY, int LZ >
__global__ __launch_bounds__( 64 * kZMarchWavesPerBlock ) void zmarch_kernel( const BrickTask* tasks, int ntasks, int xcd_chunk, const Args< OP > A )
{
   static_assert( LZ + 2 <= kBrickMaxSlices, "the table carries the slice bases of bricks of up to kBrickMaxSlices - 2 slices" );
   constexpr int NC  = OP::NC;
   constexpr int PFD = 1; // loads run one slice ahead
   int           b   = blockIdx.x;
   if ( xcd_chunk > 0 )
      b = ( blockIdx.x & 7 ) * xcd_chunk + ( blockIdx.x >> 3 );
   const int task = __builtin_amdgcn_readfirstlane( b * kZMarchWavesPerBlock + ( threadIdx.x >> 6 ) );
   if ( task >= ntasks )
      return;
   const BrickTask t    = tasks[task];
   const int       lane = threadIdx.x & 63;

   constexpr int          kStAux = 2; // nontemporal
   __amdgpu_buffer_rsrc_t rs[NC + 1], rd[NC], rr[NC], ri[NC]; // sources (NC: the coefficient), destinations, rhs, inverse diagonals
#pragma unroll
   for ( int c = 0; c < NC; ++c )
   {
      rs[c] = __builtin_amdgcn_make_buffer_rsrc( const_cast< double* >( A.src[c] ), 0, A.bytes, 0x00020000 );
      rd[c] = __builtin_amdgcn_make_buffer_rsrc( A.dst[c], 0, A.bytes, 0x00020000 );
      // rr: the rhs, or the x of CHEB_STEP (its second store stream)
      rr[c] = __builtin_amdgcn_make_buffer_rsrc( const_cast< double* >( MODE == CHEB_STEP ? A.x[c] : ( reads_rhs( MODE ) ? A.rhs[c] : A.src[c] ) ), 0,
                                                 A.bytes, 0x00020000 );
      ri[c] = __builtin_amdgcn_make_buffer_rsrc( const_cast< double* >( reads_invdiag( MODE ) ? A.invdiag[c] : A.src[c] ), 0, A.bytes, 0x00020000 );
   }
   rs[NC] = __builtin_amdgcn_make_buffer_rsrc( const_cast< double* >( A.coef ), 0, A.bytes, 0x00020000 );

   const int lane_off = lane * 8;
   const int ym       = t.y0 - 1;

   // S[c][q][r]: the sources and the coefficient ( c = NC ) at slice z0-1+q, row ym+r, x = xb + lane.  Lanes beyond the end of a
   // row re-read its last entry; a row that does not exist has a negative bound and is dropped by the range check (as in zmarch_body).
   double S[NC + 1][LZ + 2][NY + 2];
   auto   load_slice = [&]( auto qc, int base_q, int W_q ) {
      constexpr int q  = decltype( qc )::value;
      int           ix = base_q;
#pragma unroll
      for ( int r = 0; r < NY + 2; ++r )
      {
         const bool need = ( q == 0 ) ? ( r >= 1 ) : ( q == LZ + 1 ? ( r <= NY ) : true );
         if ( need )
         {
            const int last8 = ( W_q - ( ym + r ) - 1 - t.xb ) * 8;
            const int vo    = min( lane_off, last8 );
#pragma unroll
            for ( int c = 0; c < NC + 1; ++c )
               S[c][q][r] = zm_load2< double >( rs[c], vo, ix * 8 );
         }
         ix += W_q - ( ym + r );
      }
   };
   int baseq[LZ + 2], Wqs[LZ + 2];
#pragma unroll
   for ( int q = 0; q < LZ + 2; ++q )
   {
      baseq[q] = t.base[q];
      Wqs[q]   = t.W0 - q;
   }
   [&]< int... Is >( std::integer_sequence< int, Is... > ) { ( load_slice( std::integral_constant< int, Is >{}, baseq[Is], Wqs[Is] ), ... ); }
   ( std::make_integer_sequence < int, ( 2 + PFD <= LZ + 2 ? 2 + PFD : LZ + 2 ) > {} );

   // the further arrays of every mode but Replace at the output points, PFD slices ahead of their use like the source slices
   double EX0[NC][LZ][NY], EX1[NC][LZ][NY];
   auto   load_extra = [&]( auto sc ) {
      constexpr int s = decltype( sc )::value;
      constexpr int q = s + 1;
      if constexpr ( MODE != REPLACE )
      {
         const int W  = Wqs[q];
         int       ie = baseq[q] + ( W - ym ); // (xb, y0, z)
#pragma unroll
         for ( int j = 0; j < NY; ++j )
         {
            const int last8 = ( W - ( t.y0 + j ) - 1 - t.xb ) * 8;
            const int vo    = min( lane_off, last8 );
#pragma unroll
            for ( int c = 0; c < NC; ++c )
            {
               if constexpr ( MODE == ADD )
                  EX0[c][s][j] = zm_load2< double, 2 >( rd[c], vo, ie * 8 ); // read once, rewritten right after: nontemporal
               else if constexpr ( MODE == CHEB_STEP )
               {
                  EX0[c][s][j] = zm_load2< double, 2 >( rr[c], vo, ie * 8 ); // x: as Add's dst
                  EX1[c][s][j] = zm_load2< double >( ri[c], vo, ie * 8 );
               }
               else
               {
                  EX0[c][s][j] = zm_load2< double >( rr[c], vo, ie * 8 );
                  if constexpr ( reads_invdiag( MODE ) )
                     EX1[c][s][j] = zm_load2< double >( ri[c], vo, ie * 8 );
               }
            }
            ie += W - ( t.y0 + j );
         }
      }
   };
   if constexpr ( MODE != REPLACE )
   {
      [&]< int... Is >( std::integer_sequence< int, Is... > ) { ( load_extra( std::integral_constant< int, Is >{} ), ... ); }
      ( std::make_integer_sequence < int, ( PFD < LZ ? PFD : LZ ) > {} );
   }

   auto step = [&]( auto sc ) {
      constexpr int s = decltype( sc )::value; // output slice z0 + s, centre q = s + 1
      constexpr int q = s + 1;
      if constexpr ( q + 1 + PFD <= LZ + 1 )
         load_slice( std::integral_constant< int, q + 1 + PFD >{}, baseq[q + 1 + PFD], Wqs[q + 1 + PFD] );
      if constexpr ( s + PFD < LZ )
         load_extra( std::integral_constant< int, s + PFD >{} );

      const int W  = Wqs[q];
      int       io = baseq[q] + ( W - ym ); // (xb, y0, z)
#pragma unroll
      for ( int j = 0; j < NY; ++j )
      {
         double u[NC][15], k[15], a0[NC];
#pragma unroll
         for ( int c = 0; c < NC; ++c )
            gather< q >( S[c], j, u[c] );
         gather< q >( S[NC], j, k );
#pragma unroll
         for ( int c = 0; c < NC; ++c )
         {
            a0[c] = u[c][7];
#pragma unroll
            for ( int n = 0; n < 15; ++n )
               u[c][n] = u[c][n] - a0[c]; // the differences u_j - u_p
         }
         double acc[NC] = {};
         inner_sum< OP >( A, u, k, acc, std::make_integer_sequence< int, 24 >{} );

         const int R = W - ( t.y0 + j );
         // outputs are lanes 1 .. min( 62, R - 2 - xb ) of slices that exist
         const int      cnt = s < t.nz ? min( 62, R - 2 - t.xb ) : 0; // wave-uniform
         const unsigned lm1 = (unsigned) ( lane - 1 );
         const bool     on  = lm1 < (unsigned) max( cnt, 0 );
#pragma unroll
         for ( int c = 0; c < NC; ++c )
         {
            double out;
            if constexpr ( MODE == REPLACE )
               out = acc[c];
            else if constexpr ( MODE == ADD )
               out = acc[c] + EX0[c][s][j];
            else if constexpr ( MODE == JACOBI )
               out = a0[c] + A.omega * ( EX1[c][s][j] * ( EX0[c][s][j] - acc[c] ) );
            else if constexpr ( MODE == RESIDUAL )
               out = EX0[c][s][j] - acc[c];
            else if constexpr ( MODE == CHEB_START )
               out = EX1[c][s][j] * ( EX0[c][s][j] - acc[c] );
            else
               out = EX1[c][s][j] * acc[c];
            const bool write = on && ( NC == 1 || ( ( A.comps >> c ) & 1u ) );
            zm_store2< double, kStAux >( rd[c], write ? lane_off : -8, io * 8, out );
            if constexpr ( MODE == CHEB_STEP )
            {
               const double xp = A.hasPrev ? EX0[c][s][j] + A.cPrev * a0[c] : EX0[c][s][j];
               zm_store2< double, kStAux >( rr[c], write ? lane_off : -8, io * 8, xp + A.cCur * out );
            }
         }
         io += R;
      }
   };
   [&]< int... Is >( std::integer_sequence< int, Is... > ) { ( step( std::integral_constant< int, Is >{} ), ... ); }
   ( std::make_integer_sequence< int, LZ >{} );
}

// this cell's share at point (x, y, z): the sum over those of the 24 micro-cells at the point that lie inside the macro-cell.
// acc: the components of the apply ( DIAG == false ) or the diagonal entries of A^{ii} ( DIAG == true ).
template < class OP, bool DIAG >
__device__ inline void point_share( const Args< OP >& A, int x, int y, int z, double ( &acc )[OP::NC] )
{
   constexpr int NC = OP::NC;
   const int     N  = A.N;
   const int     i0 = cell_index( N, x, y, z );
   const int     w  = N - z;
   const double  kp = A.coef[i0];
   double        up[NC];
#pragma unroll
   for ( int c = 0; c < NC; ++c )
   {
      up[c]  = DIAG ? 0.0 : A.src[c][i0];
      acc[c] = 0.0;
   }
#pragma unroll
   for ( int t = 0; t < 6; ++t )
#pragma unroll
      for ( int i = 0; i < 4; ++i )
      {
         // the type-t micro-cell with the point as local vertex i: all four vertices inside the macro-cell?
         bool inside = true;
         int  idx[4];
#pragma unroll
         for ( int j = 0; j < 4; ++j )
         {
            const int dx = micro_vert( t, j, 0 ) - micro_vert( t, i, 0 ), dy = micro_vert( t, j, 1 ) - micro_vert( t, i, 1 ),
                      dz = micro_vert( t, j, 2 ) - micro_vert( t, i, 2 );
            const int nx = x + dx, ny = y + dy, nz = z + dz;
            inside       = inside && nx >= 0 && ny >= 0 && nz >= 0 && nx + ny + nz <= N - 1;
            // layout algebra of shell::share
            const int rowDelta   = dy == 0 ? 0 : ( dy > 0 ? ( w - y ) : -( w - y + 1 ) );
            const int sliceDelta = dz == 0 ? 0 : ( dz > 0 ? tri( w ) - ny : ny - tri( w + 1 ) );
            idx[j]               = i0 + sliceDelta + rowDelta + dx;
         }
         if ( !inside )
            continue;
         // m: the coefficient summed over the cell's vertices; d[c][j]: the difference of component c to vertex j ( j != i )
         double m = kp, d[NC][4] = {};
#pragma unroll
         for ( int j = 0; j < 4; ++j )
            if ( j != i )
            {
               m += A.coef[idx[j]];
               if ( !DIAG )
#pragma unroll
                  for ( int c = 0; c < NC; ++c )
                     d[c][j] = A.src[c][idx[j]] - up[c];
            }
         OP::template point_cell< DIAG >( A, t, i, m, d, acc );
      }
}

constexpr int kPointThreads = 256;

// the shell classes of A.masks (enumeration of shell.hpp); a component is written where its own mask selects the point's class
template < class OP, int MODE >
__global__ __launch_bounds__( kPointThreads ) void shell_kernel( const Args< OP > A )
{
   constexpr int NC = OP::NC;
   const int     q  = blockIdx.x * kPointThreads + threadIdx.x;
   int           x, y, z, slot;
   unsigned      any = 0;
#pragma unroll
   for ( int c = 0; c < NC; ++c )
      any |= A.masks[c];
   if ( !shell::shell_point( A.N, q, x, y, z, slot ) || !( ( any >> slot ) & 1u ) )
      return;
   double acc[NC];
   point_share< OP, MODE == DIAG >( A, x, y, z, acc );
   const int i = cell_index( A.N, x, y, z );
#pragma unroll
   for ( int c = 0; c < NC; ++c )
      if ( ( A.masks[c] >> slot ) & 1u )
         A.dst[c][i] = MODE == REPLACE ? acc[c] : acc[c] + A.dst[c][i];
}

// the inner points, one thread per point over the inner tiles (the diagonals; the comparison form of the z-march)
template < class OP, int MODE >
__global__ __launch_bounds__( kPointThreads ) void inner_point_kernel( const Args< OP > A, const Tile* tiles, int ntiles )
{
   constexpr int NC = OP::NC;
   const int     tt = blockIdx.x;
   if ( tt >= ntiles )
      return;
   const Tile tl = tiles[tt];
   const int  N = A.N, W = N - tl.z, s0 = slice_start( N, tl.z );
   for ( int e = threadIdx.x; e < tl.cnt; e += kPointThreads )
   {
      const int i = tl.a + e, j = i - s0;
      const int y = row_of( W, j ), x = j - row_start( W, y );
      if ( x < 1 || y < 1 || tl.z < 1 || x + y + tl.z > N - 2 )
         continue;
      double acc[NC];
      point_share< OP, MODE == DIAG >( A, x, y, tl.z, acc );
#pragma unroll
      for ( int c = 0; c < NC; ++c )
      {
         if ( NC > 1 && !( ( A.comps >> c ) & 1u ) )
            continue;
         double out;
         if ( MODE == REPLACE )
            out = acc[c];
         else if ( MODE == JACOBI )
            out = A.src[c][i] + A.omega * ( A.invdiag[c][i] * ( A.rhs[c][i] - acc[c] ) );
         else if ( MODE == RESIDUAL )
            out = A.rhs[c][i] - acc[c];
         else if ( MODE == CHEB_START )
            out = A.invdiag[c][i] * ( A.rhs[c][i] - acc[c] );
         else if ( MODE == CHEB_STEP )
         {
            out             = A.invdiag[c][i] * acc[c];
            const double xp = A.hasPrev ? A.x[c][i] + A.cPrev * A.src[c][i] : A.x[c][i];
            A.x[c][i]       = xp + A.cCur * out;
         }
         else
            out = acc[c] + A.dst[c][i];
         A.dst[c][i] = out;
      }
   }
}

} // namespace varcoef
} // namespace hyteg_hip
