// p1p2conversion.hpp -- part of the C++ host layer above the C-ABI (see hyteg_host.hpp for the data model).
// P1toP2Conversion / P2toP1Conversion (src/hyteg/gridtransferoperators/P1toP2Conversion.cpp:28-149, P2toP1Conversion.cpp:28-150)
// and P1toP1QuadraticProlongationThroughP2Injection (P1toP1QuadraticProlongationThroughP2Injection.hpp:33-55)
#pragma once

#include "p2gridtransfer.hpp"

namespace hyteg {

// The P2 function of level P2Level := the P1 function of level P2Level + 1 on the DoFs `flag` selects: a copy, DoF by DoF
// (hyteg_hip_p1_to_p2_cells: one launch per chunk of cells at every level).  The flag is translated with the SOURCE function's
// boundary condition, as in the reference (P1toP2Conversion.cpp:36).  No exchange follows: the copies of a shared DoF are moved
// cell by cell, so copies that were bit-identical stay so.
inline void P1toP2Conversion( const P1Function< double >& src, const P2Function< double >& dst, const uint_t& P2Level, const Selection& flag = All )
{
   auto        storage = src.getStorage();
   ScopedTimer timer( storage->getTimingTree(), "P1toP2Conversion" );
   const auto  masks = storage->masksFor( src.effectiveFlag( flag ) );
   storage->forCellChunks( [&]( int first, int count ) {
      const auto v = dst.getVertexDoFFunction().cellPointers( P2Level, first, count ), e = dst.edgeCellPointers( P2Level, first, count ),
                 p = src.cellPointers( P2Level + 1, first, count );
      hipCheck( hyteg_hip_p1_to_p2_cells( count, v.data(), e.data(), p.data(), (int) P2Level, masks.data() + first, storage->stream() ),
                "P1toP2Conversion" );
   } );
}

// The P1 function of level P1Level := the P2 function of level P1Level - 1 (the reference's level convention: this one takes the
// P1 level, P2toP1Conversion.cpp:28-31)
inline void P2toP1Conversion( const P2Function< double >& src, const P1Function< double >& dst, const uint_t& P1Level, const Selection& flag = All )
{
   if ( P1Level == 0 )
      throw std::runtime_error( "P2toP1Conversion: the P1 level must be at least 1" );
   auto         storage = src.getStorage();
   ScopedTimer  timer( storage->getTimingTree(), "P2toP1Conversion" );
   const uint_t P2Level = P1Level - 1;
   const auto   masks   = storage->masksFor( src.getVertexDoFFunction().effectiveFlag( flag ) );
   storage->forCellChunks( [&]( int first, int count ) {
      const auto v = src.getVertexDoFFunction().cellPointers( P2Level, first, count ), e = src.edgeCellPointers( P2Level, first, count ),
                 p = dst.cellPointers( P1Level, first, count );
      hipCheck( hyteg_hip_p2_to_p1_cells( count, p.data(), v.data(), e.data(), (int) P2Level, masks.data() + first, storage->stream() ),
                "P2toP1Conversion" );
   } );
}

// Quadratic prolongation of a P1 function in 3D: the P1 function of level L is read as a P2 function of level L - 1, prolongated
// with P2toP2QuadraticProlongation, and the result is read back as the P1 function of level L + 1 -- one order higher than
// P1toP1LinearProlongation, what a full multigrid pass needs to keep the discretisation accuracy.
class P1toP1QuadraticProlongationThroughP2Injection
{
 public:
   // The reference checks p1MinLevel > 2; nothing here needs more than a P2 level p1MinLevel - 1 >= 0.
   P1toP1QuadraticProlongationThroughP2Injection( const std::shared_ptr< PrimitiveStorage >& storage, const uint_t& p1MinLevel, const uint_t& p1MaxLevel )
   : tmp_( "tmp", requireLevels( storage, p1MinLevel, p1MaxLevel ), p1MinLevel - 1, p1MaxLevel - 1 )
   {}

   // The last conversion is `All`, as in the reference: the DoFs of level sourceLevel + 1 that `flag` excludes are overwritten with
   // what the temporary holds there -- zero, since nothing ever writes them.  A caller restores Dirichlet values afterwards (the
   // post-prolongate callback of FullMultigridSolver is the place).
   void prolongate( const P1Function< double >& function, const uint_t& sourceLevel, const Selection& flag ) const
   {
      if ( sourceLevel == 0 )
         throw std::runtime_error( "P1toP1QuadraticProlongationThroughP2Injection: the source level must be at least 1" );
      P1toP2Conversion( function, tmp_, sourceLevel - 1, All );
      quadraticProlongation_.prolongate( tmp_, sourceLevel - 1, flag );
      P2toP1Conversion( tmp_, function, sourceLevel + 1, All );
   }

 private:
   static const std::shared_ptr< PrimitiveStorage >& requireLevels( const std::shared_ptr< PrimitiveStorage >& storage, uint_t p1MinLevel, uint_t p1MaxLevel )
   {
      if ( p1MinLevel < 1 || p1MaxLevel < p1MinLevel )
         throw std::runtime_error( "P1toP1QuadraticProlongationThroughP2Injection: needs 1 <= p1MinLevel <= p1MaxLevel" );
      return storage;
   }
   P2Function< double >        tmp_;
   P2toP2QuadraticProlongation quadraticProlongation_;
};

} // namespace hyteg
