// P1toP2Conversion / P2toP1Conversion on the macro-cells of a rank
//   src/hyteg/gridtransferoperators/P1toP2Conversion.cpp:28-149, P2toP1Conversion.cpp:28-150 (the macro-cell loops; the reference
//   walks the P2 DoFs of every primitive and copies value by value)
// A P2 function of level L and a P1 function of level L + 1 have the same DoFs: the point ( X, Y, Z ) of the fine vertex array is
// the P2 DoF with logical index ( X >> 1, Y >> 1, Z >> 1 ) whose kind the parities of ( X, Y, Z ) select -- an edge DoF sits at the
// midpoint of its edge, 2 * index + the sum of its two end-point offsets (kEdgeEnds, p2_common.hpp).  The conversion is that
// permutation: no arithmetic, 8 bytes read and 8 bytes written per DoF.
//
// By fine rows: the points with fixed ( Y, Z ) are R = Nf - Y - Z consecutive entries of the fine array, and they are exactly two
// contiguous coarse rows -- even X: the vertex, Y, Z or YZ row ( Y >> 1, Z >> 1 ), odd X: the X, XY, XZ or XYZ row.  One wave owns one
// fine row and walks it in runs of 128 entries, two per lane ( X = x0 + 2 lane and + 1 ): on the coarse side lane l touches entry
// ( x0 >> 1 ) + l of either row, consecutive lanes consecutive addresses; the row's ( Y, Z ), kinds and the three row bases are the
// wave's.  Rows of the tetrahedral layout start at any multiple of 8 bytes, so every access is one 8-byte access (a lane's two fine
// entries are adjacent, but their pair is 16-byte aligned in every other row only).
// Included from p2_transfer.hip, whose layout helper width_of_kind it uses.
#pragma once

namespace {

struct P1P2ConversionArgs
{
   double*  p1[HYTEG_HIP_MAX_BATCH]; // level L + 1
   double*  p2v[HYTEG_HIP_MAX_BATCH];
   double*  p2e[HYTEG_HIP_MAX_BATCH];
   unsigned mask[HYTEG_HIP_MAX_BATCH]; // point classes of the destination DoFs; 0: the cell is skipped
   int      Nc, Nf;                    // widths of the P2 level's and of the P1 level's vertex array
   int      edgeBlock;                 // entries of one of the blocks X .. YZ of the edge array: tet( Nc - 1 )
};
static_assert( sizeof( P1P2ConversionArgs ) <= 4096, "the conversion's arguments must fit the 4 KB kernel-argument segment" );

constexpr int kConversionWaves = 4; // fine rows per workgroup, one per wave (four rows per wave were slower)

// kind of the P2 DoF at a fine point with parities ( px, py, pz ): 0 vertex, 1..7 X, Y, Z, XY, XZ, YZ, XYZ
__host__ __device__ constexpr int kind_of_parities( int px, int py, int pz )
{
   // the table { 0, 1, 2, 4, 3, 5, 6, 7 } indexed by px + 2 py + 4 pz, one hexadecimal digit per entry
   return (int) ( ( 0x76534210u >> ( 4 * ( px + 2 * py + 4 * pz ) ) ) & 7u );
}

// TO_P2: the P2 arrays are written from the P1 array, otherwise the P1 array from the P2 arrays.
// Grid ( groups of kConversionWaves values of y, z, cells ).
template < bool TO_P2 >
__global__ __launch_bounds__( 64 * kConversionWaves ) void p1p2_conversion_kernel( const P1P2ConversionArgs A )
{
   const int      cell = blockIdx.z;
   const unsigned mask = A.mask[cell];
   if ( mask == 0u )
      return; // nothing selected: the cell's arrays are not touched
   const int Nf = A.Nf, Nc = A.Nc;
   // every wave pays for its row's bases on the CU's one scalar unit: ( y, z ) come from the grid, not from decoding a row number,
   // the bases are 32-bit arithmetic, and the size of an edge block comes from the host (profiles/p1p2_conversion.txt)
   const int z = blockIdx.y;
   const int y = __builtin_amdgcn_readfirstlane( (int) ( blockIdx.x * kConversionWaves + ( threadIdx.x >> 6 ) ) );
   if ( y + z > Nf - 1 )
      return; // the grid is the square [ 0, Nf )^2 of ( y, z ), the rows are its lower triangle
   const int R = Nf - y - z; // entries of the fine row
   const int kindEven = kind_of_parities( 0, y & 1, z & 1 ), kindOdd = kind_of_parities( 1, y & 1, z & 1 );
   double* const fine = A.p1[cell] + cell_index( Nf, 0, y, z );
   // index of ( 0, y >> 1, z >> 1 ) of an edge kind in the edge array: its block, then the row in an array of the kind's width
   const auto edgeRow = [&]( int kind ) { return ( kind - 1 ) * A.edgeBlock + cell_index( width_of_kind( Nc, kind ), 0, y >> 1, z >> 1 ); };
   double* const even = kindEven == 0 ? A.p2v[cell] + cell_index( Nc, 0, y >> 1, z >> 1 ) : A.p2e[cell] + edgeRow( kindEven );
   // an XYZ row that holds no entry (R == 1) has no valid base: it is not dereferenced, no lane has an odd x < R
   double* const odd = A.p2e[cell] + ( R > 1 ? edgeRow( kindOdd ) : 0 );
   const bool    all  = ( mask & HYTEG_HIP_MASK_ALL ) == HYTEG_HIP_MASK_ALL;
   const int     lane = threadIdx.x & 63;
   for ( int x0 = 0; x0 < R; x0 += 128 )
   {
      const int  x  = x0 + 2 * lane;
      // the class of a P2 DoF is the class of the fine point it sits on (an edge DoF belongs to the primitive that holds both its
      // end points, which is the one that holds its midpoint)
      const bool s0 = x < R && ( all || ( ( mask >> point_slot< 14 >( Nf, x, y, z ) ) & 1u ) );
      const bool s1 = x + 1 < R && ( all || ( ( mask >> point_slot< 14 >( Nf, x + 1, y, z ) ) & 1u ) );
      const int  i  = x >> 1;
      if constexpr ( TO_P2 )
      {
         const double v0 = s0 ? fine[x] : 0.0, v1 = s1 ? fine[x + 1] : 0.0;
         if ( s0 )
            even[i] = v0;
         if ( s1 )
            odd[i] = v1;
      }
      else
      {
         const double v0 = s0 ? even[i] : 0.0, v1 = s1 ? odd[i] : 0.0;
         if ( s0 )
            fine[x] = v0;
         if ( s1 )
            fine[x + 1] = v1;
      }
   }
}

// both directions: every argument is checked before anything touches the GPU; one launch, nothing allocated, no synchronisation
int launch_p1p2_conversion( bool                 toP2,
                            const char*          what,
                            int                  ncells,
                            const double* const* p1,
                            const double* const* p2v,
                            const double* const* p2e,
                            int                  p2_level,
                            const unsigned*      masks,
                            hyteg_hip_stream_t   stream )
{
   const std::string name( what );
   HH_REQUIRE( ncells >= 1 && ncells <= HYTEG_HIP_MAX_BATCH, name + ": ncells must be 1..HYTEG_HIP_MAX_BATCH" );
   HH_REQUIRE( p1 && p2v && p2e && masks, name + ": null pointer" );
   HH_REQUIRE( p2_level >= 0 && p2_level <= HYTEG_HIP_P2_MAX_LEVEL, name + ": P2 level out of range [0,9]" );
   P1P2ConversionArgs A{};
   bool               any = false;
   for ( int c = 0; c < ncells; ++c )
   {
      HH_REQUIRE( p1[c] && p2v[c] && p2e[c], name + ": null array of a cell" );
      HH_REQUIRE( p1[c] != p2v[c] && p1[c] != p2e[c], name + ": the P1 array must not alias a P2 array of the same cell" );
      A.p1[c] = const_cast< double* >( p1[c] ), A.p2v[c] = const_cast< double* >( p2v[c] ), A.p2e[c] = const_cast< double* >( p2e[c] );
      A.mask[c] = masks[c] & HYTEG_HIP_MASK_ALL;
      any       = any || A.mask[c];
   }
   if ( !any )
      return HYTEG_HIP_OK;
   A.Nc = ( 1 << p2_level ) + 1, A.Nf = ( 1 << ( p2_level + 1 ) ) + 1;
   A.edgeBlock = (int) tet32( (unsigned) ( A.Nc - 1 ) );
   const dim3 grid( (unsigned) ( ( A.Nf + kConversionWaves - 1 ) / kConversionWaves ), (unsigned) A.Nf, (unsigned) ncells );
   if ( toP2 )
      hipLaunchKernelGGL( p1p2_conversion_kernel< true >, grid, dim3( 64 * kConversionWaves ), 0, as_stream( stream ), A );
   else
      hipLaunchKernelGGL( p1p2_conversion_kernel< false >, grid, dim3( 64 * kConversionWaves ), 0, as_stream( stream ), A );
   HH_CHECK_HIP( hipGetLastError() );
   return HYTEG_HIP_OK;
}

} // namespace
