// p1divkgrad.hpp -- part of the C++ host layer above the C-ABI (see hyteg_host.hpp for the data model).
// P1ElementwiseDivKGrad: the generated variable-coefficient diffusion operator -div( k grad u ) with a P1 coefficient function,
//    operatorgeneration::P1ElementwiseDivKGrad( storage, minLevel, maxLevel, const P1Function< real_t >& k )
// (module hyteg_operators; call site and known answer: tests/hyteg/convergence/ElementwiseDivKGradCGConvergenceTest.cpp:73-81,
// 175-177).  Same class shape as P1ElementwiseDiffusion (p1elementwise.hpp) plus the coefficient; the per-cell call is the C-ABI
// seam hyteg_hip_p1_elementwise_divkgrad_apply_macro_3d_masked.  The operator at level l reads k at level l: the caller
// interpolates k on every level it uses, as the reference test does.  smooth_jac is P1ElementwiseOperator::smooth_jac
// (src/hyteg/elementwiseoperators/P1ElementwiseOperator.cpp:288-331), fused into one launch on the inner points; so are the residual
// of a multigrid cycle and the steps of the Chebyshev smoother (residual, chebyshevStart / Step / Finish: what GeometricMultigridSolver
// and ChebyshevSmoother look for).
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

   // the fused Jacobi, residual and Chebyshev entries on the inner points (default), or the composed passes everywhere (tests, measurements)
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
      if ( &src == &dst || &dst == &k_ || &dst == &rhs )
         throw std::runtime_error( "P1ElementwiseDivKGrad::smooth_jac: dst must differ from src, rhs and k" );
      sharesInnerShell(
          dst, src, level, dst.effectiveFlag( flagIn ),
          [&]( uint_t c, const double* cc ) {
             hipCheck( hyteg_hip_p1_elementwise_divkgrad_jacobi_macro_3d( dst.getCellPointer( c, level ), src.getCellPointer( c, level ),
                                                                          rhs.getCellPointer( c, level ), invDiag.getCellPointer( c, level ),
                                                                          k_.getCellPointer( c, level ), cc, int64_t( 1 ) << level, omega, storage_->stream() ),
                       "P1ElementwiseDivKGrad::smooth_jac: cell" );
          },
          [&]( uint_t c, unsigned shell ) { smoothJacShellPasses( dst, rhs, invDiag, src, omega, c, level, shell ); } );
   }

   // r = b - A x as the multigrid cycle writes it (GeometricMultigridSolver.hpp:240-246: apply, then assign).  Fused: the inner
   // points in one launch per cell (hyteg_hip_p1_elementwise_divkgrad_residual_macro_3d), the shell as in smooth_jac.
   void residual( const P1Function< double >& x, const P1Function< double >& b, const P1Function< double >& r, uint_t level, const Selection& flagIn ) const
   {
      if ( !fusedOn( level ) || &x == &r )
      {
         apply( x, r, level, flagIn );
         r.assign( { 1.0, -1.0 }, { b, r }, level, flagIn );
         return;
      }
      ScopedTimer timerOp( storage_->getTimingTree(), "Operator P1Function to P1Function" ), timerRes( storage_->getTimingTree(), "residual" );
      checkOutput( "residual", r, { &b } );
      sharesInnerShell(
          r, x, level, r.effectiveFlag( flagIn ),
          [&]( uint_t c, const double* cc ) {
             hipCheck( hyteg_hip_p1_elementwise_divkgrad_residual_macro_3d( r.getCellPointer( c, level ), x.getCellPointer( c, level ),
                                                                            b.getCellPointer( c, level ), k_.getCellPointer( c, level ), cc,
                                                                            int64_t( 1 ) << level, storage_->stream() ),
                       "P1ElementwiseDivKGrad::residual: cell" );
          },
          [&]( uint_t c, unsigned shell ) { fusedStepShellPasses( r, &b, nullptr, nullptr, 0.0, c, level, shell ); } );
   }

   // ---- the steps of ChebyshevSmoother::solve (ChebyshevSmoother.hpp:165-212) with the semantics of P1ConstantOperator's
   // (p1operator.hpp): one launch per step and cell on the inner points (hyteg_hip_p1_elementwise_divkgrad_chebyshev_*_macro_3d),
   // the shell as in smooth_jac.  Where chebyshevFusable is false the smoother runs its generic sequence.
   bool chebyshevFusable( uint_t level ) const { return fusedOn( level ); }
   // t = invDiag .* ( b - A x ); on the shell also x += c0 t.  On the inner points x is this launch's stencil source: its update
   // is carried out by the following chebyshevStep( ..., hasPrev = true ) or by chebyshevFinish
   void chebyshevStart( const P1Function< double >& t, const P1Function< double >& b, const P1Function< double >& x, double c0, uint_t level,
                        const Selection& flagIn ) const
   {
      ScopedTimer timerOp( storage_->getTimingTree(), "Operator P1Function to P1Function" ), timerCheb( storage_->getTimingTree(), "chebyshev" );
      const auto& invDiag = *getInverseDiagonalValues();
      checkOutput( "chebyshevStart", t, { &b, &x, &invDiag } );
      sharesInnerShell(
          t, x, level, x.effectiveFlag( flagIn ),
          [&]( uint_t c, const double* cc ) {
             hipCheck( hyteg_hip_p1_elementwise_divkgrad_chebyshev_start_macro_3d( t.getCellPointer( c, level ), b.getCellPointer( c, level ),
                                                                                   x.getCellPointer( c, level ), invDiag.getCellPointer( c, level ),
                                                                                   k_.getCellPointer( c, level ), cc, int64_t( 1 ) << level,
                                                                                   storage_->stream() ),
                       "P1ElementwiseDivKGrad::chebyshevStart: cell" );
          },
          [&]( uint_t c, unsigned shell ) { fusedStepShellPasses( t, &b, &invDiag, &x, c0, c, level, shell ); } );
   }
   // tOut = invDiag .* ( A tIn ); x = ( x + cPrev tIn ) + cCur tOut on the inner points (first term only if hasPrev: the update
   // chebyshevStart left open), x += cCur tOut on the shell
   void chebyshevStep( const P1Function< double >& tOut, const P1Function< double >& x, const P1Function< double >& tIn, double cPrev, double cCur,
                       bool hasPrev, uint_t level, const Selection& flagIn ) const
   {
      ScopedTimer timerOp( storage_->getTimingTree(), "Operator P1Function to P1Function" ), timerCheb( storage_->getTimingTree(), "chebyshev" );
      const auto& invDiag = *getInverseDiagonalValues();
      checkOutput( "chebyshevStep", tOut, { &x, &tIn, &invDiag } );
      checkOutput( "chebyshevStep", x, { &tIn, &invDiag } );
      sharesInnerShell(
          tOut, tIn, level, x.effectiveFlag( flagIn ),
          [&]( uint_t c, const double* cc ) {
             hipCheck( hyteg_hip_p1_elementwise_divkgrad_chebyshev_step_macro_3d( tOut.getCellPointer( c, level ), x.getCellPointer( c, level ),
                                                                                  tIn.getCellPointer( c, level ), invDiag.getCellPointer( c, level ),
                                                                                  k_.getCellPointer( c, level ), cc, int64_t( 1 ) << level, cPrev, cCur,
                                                                                  hasPrev ? 1 : 0, storage_->stream() ),
                       "P1ElementwiseDivKGrad::chebyshevStep: cell" );
          },
          [&]( uint_t c, unsigned shell ) { fusedStepShellPasses( tOut, nullptr, &invDiag, &x, cCur, c, level, shell ); } );
   }
   // x += c t on the inner points: closes a smoother call of order 1 (no step follows the start)
   void chebyshevFinish( const P1Function< double >& x, const P1Function< double >& t, double c, uint_t level, const Selection& flagIn ) const
   {
      const Selection flag = x.effectiveFlag( flagIn );
      storage_->forLocalCells( [&]( uint_t ci, const MacroCell& cell ) {
         chebyshevFinishCell( x, t, c, ci, level, storage_->maskFor( cell, flag ) & HYTEG_HIP_MASK_INNER );
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
   // the fused entries act on the inner points: below level 2 there are none, and setFused( false ) composes everywhere
   bool fusedOn( uint_t level ) const { return fused_ && level >= HYTEG_HIP_MIN_LEVEL; }
   void checkOutput( const char* who, const P1Function< double >& out, std::initializer_list< const P1Function< double >* > others ) const
   {
      bool bad = &out == &k_;
      for ( const P1Function< double >* f : others )
         bad = bad || &out == f || f == &k_;
      if ( bad )
         throw std::runtime_error( std::string( "P1ElementwiseDivKGrad::" ) + who + ": a written function must differ from the others, and all from k" );
   }
   // the schedule of a fused step out = f( A src ): this cell's shares of A src on the shell classes, the additive exchange of the
   // shares while the inner points are computed by inner( cell index, macro_vertex_coords ), then shell( cell index, shell classes )
   template < class Inner, class Shell >
   void sharesInnerShell( const P1Function< double >& out, const P1Function< double >& src, uint_t level, const Selection& flag, Inner&& inner,
                          Shell&& shell ) const
   {
      storage_->forLocalCells( [&]( uint_t c, const MacroCell& cell ) {
         kernel( out, src, c, cell, level, storage_->maskFor( cell, flag ) & HYTEG_HIP_MASK_SHELL, HYTEG_HIP_REPLACE );
      } );
      out.beginSumSharedCopies( level, flag );
      storage_->forLocalCells( [&]( uint_t c, const MacroCell& cell ) {
         if ( !( storage_->maskFor( cell, flag ) & HYTEG_HIP_MASK_INNER ) || level < HYTEG_HIP_MIN_LEVEL )
            return;
         double cc[12];
         coordsOf( cell, cc );
         inner( c, cc );
      } );
      out.endSumSharedCopies( level, flag );
      storage_->forLocalCells( [&]( uint_t c, const MacroCell& cell ) { shell( c, storage_->maskFor( cell, flag ) & HYTEG_HIP_MASK_SHELL ); } );
   }
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
