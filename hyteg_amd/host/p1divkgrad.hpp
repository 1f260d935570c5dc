// p1divkgrad.hpp -- part of the C++ host layer above the C-ABI (see hyteg_host.hpp for the data model).
// P1ElementwiseDivKGrad: the generated variable-coefficient diffusion operator -div( k grad u ) with a P1 coefficient function,
//    operatorgeneration::P1ElementwiseDivKGrad( storage, minLevel, maxLevel, const P1Function< real_t >& k )
// (module hyteg_operators; call site and known answer: tests/hyteg/convergence/ElementwiseDivKGradCGConvergenceTest.cpp:73-81,
// 175-177).  Same class shape as P1ElementwiseDiffusion (p1elementwise.hpp) plus the coefficient; the per-cell call is the C-ABI
// seam hyteg_hip_p1_elementwise_divkgrad_apply_macro_3d_masked.  The operator at level l reads k at level l: the caller
// interpolates k on every level it uses, as the reference test does.  smooth_jac is P1ElementwiseOperator::smooth_jac
// (src/hyteg/elementwiseoperators/P1ElementwiseOperator.cpp:288-331), fused into one launch on the inner points.
#pragma once

#include "p1function.hpp"

namespace hyteg {
namespace operatorgeneration {

class P1ElementwiseDivKGrad
{
 public:
   using srcType = P1Function< double >;
   using dstType = P1Function< double >;

   P1ElementwiseDivKGrad( const std::shared_ptr< PrimitiveStorage >& storage, uint_t minLevel, uint_t maxLevel, const P1Function< double >& k )
   : storage_( storage )
   , minLevel_( minLevel )
   , maxLevel_( maxLevel )
   , k_( k )
   {
      if ( maxLevel > 8 )
         throw std::runtime_error( "P1ElementwiseDivKGrad: levels 0..8" );
      storage->markInUse(); // the mesh boundary flags are fixed from here on
      for ( uint_t l = std::max< uint_t >( minLevel, HYTEG_HIP_MIN_LEVEL ); l <= maxLevel; ++l )
         hipCheck( hyteg_hip_prepare_level( (int) l ), "P1ElementwiseDivKGrad: prepare_level" );
   }
   std::shared_ptr< PrimitiveStorage > getStorage() const { return storage_; }
   uint_t                              getMinLevel() const { return minLevel_; }
   uint_t                              getMaxLevel() const { return maxLevel_; }
   const P1Function< double >&         getCoefficient() const { return k_; }
   uint64_t                            uid() const { return uid_; }

   // the fused Jacobi entry on the inner points (default), or the composed four passes everywhere (tests, measurements)
   void setFused( bool on ) { fused_ = on; }
   bool getFused() const { return fused_; }

   // the schedule of P1ElementwiseDiffusion::apply: shell classes first (this cell's shares), the additive exchange of the shares
   // while the inner points are computed, Add on several cells through a scratch function
   void apply( const P1Function< double >& src, const P1Function< double >& dst, uint_t level, const Selection& flagIn, UpdateType updateType = Replace ) const
   {
      ScopedTimer timerOp( storage_->getTimingTree(), "Operator P1Function to P1Function" ), timerApply( storage_->getTimingTree(), "apply" );
      const Selection flag = dst.effectiveFlag( flagIn );
      if ( &src == &dst || &dst == &k_ )
         throw std::runtime_error( "P1ElementwiseDivKGrad::apply: dst must differ from src and from k" );
      std::unique_ptr< P1Function< double > > tmp;
      if ( updateType == Add && storage_->anyShellSelected( flag ) && ( storage_->getCells().size() > 1 ) )
         tmp = P1Function< double >::zeroedScratch( "apply_tmp", storage_, level );
      const P1Function< double >& shellDst = tmp ? *tmp : dst;
      storage_->forLocalCells( [&]( uint_t c, const MacroCell& cell ) {
         kernel( shellDst, src, c, cell, level, storage_->maskFor( cell, flag ) & HYTEG_HIP_MASK_SHELL, hipUpdate( tmp ? Replace : updateType ) );
      } );
      shellDst.beginSumSharedCopies( level, flag );
      storage_->forLocalCells( [&]( uint_t c, const MacroCell& cell ) {
         kernel( dst, src, c, cell, level, storage_->maskFor( cell, flag ) & HYTEG_HIP_MASK_INNER, hipUpdate( updateType ) );
      } );
      shellDst.endSumSharedCopies( level, flag );
      if ( tmp )
         dst.addOnShell( *tmp, level, flag );
   }

   // invDiag_ = 0; per cell computeInverseDiagonalOperatorValues_macro_3D( invDiag_, k, coordinates, micro_edges ); additive
   // communication; invertElementwise
   void computeInverseDiagonalOperatorValues()
   {
      invDiag_.reset( new P1Function< double >( "inverse diagonal entries", storage_, minLevel_, maxLevel_ ) );
      for ( uint_t l = minLevel_; l <= maxLevel_; ++l )
      {
         invDiag_->interpolate( 0.0, l, All );
         storage_->forLocalCells( [&]( uint_t c, const MacroCell& cell ) {
            double cc[12];
            coordsOf( cell, cc );
            hipCheck( hyteg_hip_p1_elementwise_divkgrad_diagonal_macro_3d( invDiag_->getCellPointer( c, l ), k_.getCellPointer( c, l ), cc,
                                                                           int64_t( 1 ) << l, storage_->stream() ),
                      "P1ElementwiseDivKGrad: diagonal" );
         } );
         invDiag_->sumSharedCopies( l, All );
         invertElementwise( *invDiag_, l );
      }
   }
   std::shared_ptr< P1Function< double > > getInverseDiagonalValues() const
   {
      if ( !invDiag_ )
         throw std::runtime_error( "Inverse diagonal values have not been assembled, call computeInverseDiagonalOperatorValues() "
                                   "to set up this function." );
      return invDiag_;
   }

   // P1ElementwiseOperator::smooth_jac, P1ElementwiseOperator.cpp:288-331:
   //   dst = A src ; dst = rhs - dst ; dst = invDiag .* dst ; dst = src + omega dst
   // Fused: the inner points in one launch per cell (hyteg_hip_p1_elementwise_divkgrad_jacobi_macro_3d); the shell points get this
   // cell's shares of A src, the additive exchange, then the reference's three vector passes restricted to the shell.
   void smooth_jac( const P1Function< double >& dst, const P1Function< double >& rhs, const P1Function< double >& src, double omega, uint_t level,
                    const Selection& flagIn ) const
   {
      ScopedTimer timerOp( storage_->getTimingTree(), "Operator P1Function to P1Function" ), timerJac( storage_->getTimingTree(), "smooth_jac" );
      const auto& invDiag = *getInverseDiagonalValues();
      if ( !fused_ )
      {
         apply( src, dst, level, flagIn, Replace );
         dst.assign( { 1.0, -1.0 }, { rhs, dst }, level, flagIn );
         dst.multElementwise( { invDiag, dst }, level, flagIn );
         dst.assign( { 1.0, omega }, { src, dst }, level, flagIn );
         return;
      }
      const Selection flag = dst.effectiveFlag( flagIn );
      if ( &src == &dst || &dst == &k_ || &dst == &rhs )
         throw std::runtime_error( "P1ElementwiseDivKGrad::smooth_jac: dst must differ from src, rhs and k" );
      storage_->forLocalCells( [&]( uint_t c, const MacroCell& cell ) {
         kernel( dst, src, c, cell, level, storage_->maskFor( cell, flag ) & HYTEG_HIP_MASK_SHELL, HYTEG_HIP_REPLACE );
      } );
      dst.beginSumSharedCopies( level, flag );
      storage_->forLocalCells( [&]( uint_t c, const MacroCell& cell ) {
         if ( !( storage_->maskFor( cell, flag ) & HYTEG_HIP_MASK_INNER ) || level < HYTEG_HIP_MIN_LEVEL )
            return;
         double cc[12];
         coordsOf( cell, cc );
         hipCheck( hyteg_hip_p1_elementwise_divkgrad_jacobi_macro_3d( dst.getCellPointer( c, level ), src.getCellPointer( c, level ),
                                                                      rhs.getCellPointer( c, level ), invDiag.getCellPointer( c, level ),
                                                                      k_.getCellPointer( c, level ), cc, int64_t( 1 ) << level, omega, storage_->stream() ),
                   "P1ElementwiseDivKGrad::smooth_jac: cell" );
      } );
      dst.endSumSharedCopies( level, flag );
      storage_->forLocalCells( [&]( uint_t c, const MacroCell& cell ) {
         smoothJacShellPasses( dst, rhs, invDiag, src, omega, c, level, storage_->maskFor( cell, flag ) & HYTEG_HIP_MASK_SHELL );
      } );
   }

   // what CGSolver asks of an operator on P1 functions: this one has no single-launch solve of small levels
   bool canCgSolveSmall( uint_t ) const { return false; }
   bool cgSmallClassesFit( const P1Function< double >&, uint_t, const Selection& ) const { return false; }
   void cgSolveSmall( const P1Function< double >&, const P1Function< double >&, uint_t, const Selection&, uint_t, double, double, double* ) const
   {
      throw std::runtime_error( "P1ElementwiseDivKGrad: no single-launch CG" );
   }

 private:
   void kernel( const P1Function< double >& out, const P1Function< double >& src, uint_t c, const MacroCell& cell, uint_t level, unsigned mask,
                int update ) const
   {
      if ( mask == 0 )
         return;
      double cc[12];
      coordsOf( cell, cc );
      hipCheck( hyteg_hip_p1_elementwise_divkgrad_apply_macro_3d_masked( out.getCellPointer( c, level ), src.getCellPointer( c, level ),
                                                                         k_.getCellPointer( c, level ), cc, int64_t( 1 ) << level, mask, update,
                                                                         storage_->stream() ),
                "P1ElementwiseDivKGrad::apply: apply_macro_3D" );
   }

   std::shared_ptr< PrimitiveStorage >     storage_;
   uint_t                                  minLevel_, maxLevel_;
   const P1Function< double >&             k_;
   uint64_t                                uid_ = nextUid();
   bool                                    fused_ = true;
   std::shared_ptr< P1Function< double > > invDiag_;
};

} // namespace operatorgeneration
} // namespace hyteg
