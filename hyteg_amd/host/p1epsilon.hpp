// p1epsilon.hpp -- part of the C++ host layer above the C-ABI (see hyteg_host.hpp for the data model).
// Variable-viscosity Stokes for P1-P1:
//   P1ElementwiseAffineEpsilonOperator( storage, minLevel, maxLevel, mu )            src/mixed_operator/P1EpsilonOperator.hpp:89-164
//   P1P1ElementwiseAffineEpsilonStokesOperator( storage, minLevel, maxLevel, mu )    src/mixed_operator/P1P1ElementwiseAffineEpsilonStokesOperator.hpp:32-92
// and the pressure preconditioner weighted with the viscosity.  The reference takes the viscosity as a std::function sampled at
// the four points of a degree-2 rule; here it is a P1Function (as the coefficient of P1ElementwiseDivKGrad): the two operators
// coincide where mu is linear on every micro-cell, in particular for mu = 1 of the reference's convergence test
// (tests/hyteg/convergence/ElementwiseEpsilonMinResConvergenceTest.cpp).  The operator at level l reads mu at level l.
// The reference composes the velocity block of nine P1ElementwiseOperator blocks (nine applies per macro-cell); here one C-ABI call
// per macro-cell and kernel kind computes the three components (hyteg_hip_p1_elementwise_epsilon_*).
// The operator also offers what GeometricMultigridSolver and ChebyshevSmoother look for (residual, chebyshevStart / Step / Finish, each
// one fused launch on the inner points), so a multigrid cycle runs on it with P1VectorFunctionLinearRestriction / Prolongation
// (stokes.hpp), and StokesVectorBlockDiagonalPreconditioner (minres.hpp) makes that cycle the velocity action of a MINRES preconditioner.
#pragma once

#include "stokes.hpp"

namespace hyteg {

class P1ElementwiseAffineEpsilonOperator
{
 public:
   using srcType = P1VectorFunction< double >;
   using dstType = P1VectorFunction< double >;

   P1ElementwiseAffineEpsilonOperator( const std::shared_ptr< PrimitiveStorage >& storage, uint_t minLevel, uint_t maxLevel, const P1Function< double >& mu )
   : storage_( storage )
   , minLevel_( minLevel )
   , maxLevel_( maxLevel )
   , mu_( mu )
   {
      if ( maxLevel > 8 )
         throw std::runtime_error( "P1ElementwiseAffineEpsilonOperator: levels 0..8" );
      storage->markInUse(); // the mesh boundary flags are fixed from here on
      for ( uint_t l = std::max< uint_t >( minLevel, HYTEG_HIP_MIN_LEVEL ); l <= maxLevel; ++l )
         hipCheck( hyteg_hip_prepare_level( (int) l ), "P1ElementwiseAffineEpsilonOperator: prepare_level" );
   }
   std::shared_ptr< PrimitiveStorage > getStorage() const { return storage_; }
   uint_t                              getMinLevel() const { return minLevel_; }
   uint_t                              getMaxLevel() const { return maxLevel_; }
   const P1Function< double >&         getViscosity() const { return mu_; }
   uint64_t                            uid() const { return uid_; }

   // the fused Jacobi, residual and Chebyshev entries on the inner points (default), or the composed passes everywhere (tests, measurements)
   void setFused( bool on ) { fused_ = on; }
   bool getFused() const { return fused_; }

   // The schedule of P1ElementwiseDivKGrad::apply for the three components in one pass: shell classes first (this cell's shares),
   // the additive exchange of the shares, the inner points, Add on several cells through scratch functions.  Every component
   // has its own boundary condition (VectorToVectorOperator applies block ( i, j ) with the flag on dst[i]): the kernels take a class
   // mask per component and leave a point that a component's condition excludes unwritten in that component.
   void apply( const srcType& src, const dstType& dst, uint_t level, const Selection& flagIn, UpdateType updateType = Replace ) const
   {
      ScopedTimer     timerOp( storage_->getTimingTree(), "Operator P1VectorFunction to P1VectorFunction" ), timerApply( storage_->getTimingTree(), "apply" );
      const Selection flag[3] = { dst[0].effectiveFlag( flagIn ), dst[1].effectiveFlag( flagIn ), dst[2].effectiveFlag( flagIn ) };
      checkDistinct( "apply", dst, { &src } );
      const bool anyShell = storage_->anyShellSelected( flag[0] ) || storage_->anyShellSelected( flag[1] ) || storage_->anyShellSelected( flag[2] );
      std::unique_ptr< P1Function< double > > tmp[3];
      if ( updateType == Add && anyShell && ( storage_->getCells().size() > 1 ) )
         for ( uint_t k = 0; k < 3; ++k )
            tmp[k] = P1Function< double >::zeroedScratch( "apply_tmp", storage_, level );
      const P1Function< double >* shellDst[3];
      for ( uint_t k = 0; k < 3; ++k )
         shellDst[k] = tmp[k] ? tmp[k].get() : &dst[k];
      storage_->forLocalCells( [&]( uint_t c, const MacroCell& cell ) {
         kernel( shellDst, src, c, cell, level, flag, HYTEG_HIP_MASK_SHELL, hipUpdate( tmp[0] ? Replace : updateType ) );
      } );
      // the exchange plans of a level are shared by all functions: one exchange in flight at a time; the first overlaps the inner points
      shellDst[0]->beginSumSharedCopies( level, flag[0] );
      const P1Function< double >* innerDst[3] = { &dst[0], &dst[1], &dst[2] };
      storage_->forLocalCells(
          [&]( uint_t c, const MacroCell& cell ) { kernel( innerDst, src, c, cell, level, flag, HYTEG_HIP_MASK_INNER, hipUpdate( updateType ) ); } );
      shellDst[0]->endSumSharedCopies( level, flag[0] );
      for ( uint_t k = 1; k < 3; ++k )
         shellDst[k]->sumSharedCopies( level, flag[k] );
      if ( tmp[0] )
         for ( uint_t k = 0; k < 3; ++k )
            dst[k].addOnShell( *tmp[k], level, flag[k] );
   }

   // VectorToVectorOperator::computeInverseDiagonalOperatorValues + extractInverseDiagonal: the inverse diagonals of the three
   // diagonal blocks.  Per level: zero; per cell the diagonal kernel; additive communication; invertElementwise
   void computeInverseDiagonalOperatorValues()
   {
      invDiag_.reset( new P1VectorFunction< double >( "inverse diagonal entries", storage_, minLevel_, maxLevel_ ) );
      for ( uint_t l = minLevel_; l <= maxLevel_; ++l )
      {
         invDiag_->interpolate( 0.0, l, All );
         storage_->forLocalCells( [&]( uint_t c, const MacroCell& cell ) {
            double cc[12];
            coordsOf( cell, cc );
            double* d[3] = { ( *invDiag_ )[0].getCellPointer( c, l ), ( *invDiag_ )[1].getCellPointer( c, l ), ( *invDiag_ )[2].getCellPointer( c, l ) };
            hipCheck( hyteg_hip_p1_elementwise_epsilon_diagonal_macro_3d( d, mu_.getCellPointer( c, l ), cc, int64_t( 1 ) << l, storage_->stream() ),
                      "P1ElementwiseAffineEpsilonOperator: diagonal" );
         } );
         for ( uint_t k = 0; k < 3; ++k )
         {
            ( *invDiag_ )[k].sumSharedCopies( l, All );
            invertElementwise( ( *invDiag_ )[k], l );
         }
      }
   }
   bool                                          hasInverseDiagonalValues() const { return invDiag_ != nullptr; }
   std::shared_ptr< P1VectorFunction< double > > getInverseDiagonalValues() const
   {
      if ( !invDiag_ )
         throw std::runtime_error( "Inverse diagonal values have not been assembled, call computeInverseDiagonalOperatorValues() "
                                   "to set up this function." );
      return invDiag_;
   }

   // P1ElementwiseOperator::smooth_jac (P1ElementwiseOperator.cpp:288-331) on the three components:
   //   dst = A src ; dst = rhs - dst ; dst = invDiag .* dst ; dst = src + omega dst
   // Fused: the inner points of the three components in one launch per cell (hyteg_hip_p1_elementwise_epsilon_jacobi_macro_3d); the
   // shell points get this cell's shares of A src, the additive exchange, then the reference's three vector passes on the shell.
   void smooth_jac( const dstType& dst, const srcType& rhs, const srcType& src, double omega, uint_t level, const Selection& flagIn ) const
   {
      ScopedTimer timerOp( storage_->getTimingTree(), "Operator P1VectorFunction to P1VectorFunction" ), timerJac( storage_->getTimingTree(), "smooth_jac" );
      const auto&     invDiag = *getInverseDiagonalValues();
      const Selection flag[3] = { dst[0].effectiveFlag( flagIn ), dst[1].effectiveFlag( flagIn ), dst[2].effectiveFlag( flagIn ) };
      // the fused launch writes the inner points of all three components: composed where their conditions disagree on a cell
      bool fused = fused_;
      storage_->forLocalCells( [&]( uint_t, const MacroCell& cell ) {
         const unsigned i0 = storage_->maskFor( cell, flag[0] ) & HYTEG_HIP_MASK_INNER;
         fused = fused && i0 == ( storage_->maskFor( cell, flag[1] ) & HYTEG_HIP_MASK_INNER ) &&
                 i0 == ( storage_->maskFor( cell, flag[2] ) & HYTEG_HIP_MASK_INNER );
      } );
      if ( !fused )
      {
         apply( src, dst, level, flagIn, Replace );
         for ( uint_t k = 0; k < 3; ++k )
         {
            dst[k].assign( { 1.0, -1.0 }, { rhs[k], dst[k] }, level, flagIn );
            dst[k].multElementwise( { invDiag[k], dst[k] }, level, flagIn );
            dst[k].assign( { 1.0, omega }, { src[k], dst[k] }, level, flagIn );
         }
         return;
      }
      checkDistinct( "smooth_jac", dst, { &src, &rhs } );
      sharesInnerShell(
          dst, src, level, flag,
          [&]( uint_t c, const double* cc, unsigned ) {
             double*       d[3];
             const double *s[3], *r[3], *i[3];
             cellPointers( dst, c, level, d ), cellPointers( src, c, level, s ), cellPointers( rhs, c, level, r ), cellPointers( invDiag, c, level, i );
             hipCheck( hyteg_hip_p1_elementwise_epsilon_jacobi_macro_3d( d, s, r, i, mu_.getCellPointer( c, level ), cc, int64_t( 1 ) << level, omega,
                                                                         storage_->stream() ),
                       "P1ElementwiseAffineEpsilonOperator::smooth_jac: cell" );
          },
          [&]( uint_t k, uint_t c, unsigned shell ) { smoothJacShellPasses( dst[k], rhs[k], invDiag[k], src[k], omega, c, level, shell ); } );
   }

   // r = b - A x as the multigrid cycle writes it (GeometricMultigridSolver.hpp:240-246: apply, then assign, over three components).
   // Fused: the inner points of the three components in one launch per cell (hyteg_hip_p1_elementwise_epsilon_residual_macro_3d), the
   // shell as in smooth_jac.  A component whose condition does not select a cell's inner points is left out of that launch (comps).
   void residual( const srcType& x, const srcType& b, const dstType& r, uint_t level, const Selection& flagIn ) const
   {
      // views of the same functions are different VectorFunction objects (the C facade builds one per argument): compare components
      bool inPlace = false;
      for ( uint_t i = 0; i < 3; ++i )
         for ( uint_t j = 0; j < 3; ++j )
            inPlace = inPlace || &x[i] == &r[j];
      if ( !fusedOn( level ) || inPlace )
      {
         apply( x, r, level, flagIn );
         for ( uint_t k = 0; k < 3; ++k )
            r[k].assign( { 1.0, -1.0 }, { b[k], r[k] }, level, flagIn ); // the whole Selection, under r[k]'s condition as in the fused path
         return;
      }
      ScopedTimer timerOp( storage_->getTimingTree(), "Operator P1VectorFunction to P1VectorFunction" ), timerRes( storage_->getTimingTree(), "residual" );
      checkDistinct( "residual", r, { &x, &b } );
      const auto flag = r.effectiveFlag( flagIn );
      sharesInnerShell(
          r, x, level, flag.data(),
          [&]( uint_t c, const double* cc, unsigned comps ) {
             double*       d[3];
             const double *s[3], *f[3];
             cellPointers( r, c, level, d ), cellPointers( x, c, level, s ), cellPointers( b, c, level, f );
             hipCheck( hyteg_hip_p1_elementwise_epsilon_residual_macro_3d( d, s, f, mu_.getCellPointer( c, level ), cc, int64_t( 1 ) << level, comps,
                                                                           storage_->stream() ),
                       "P1ElementwiseAffineEpsilonOperator::residual: cell" );
          },
          [&]( uint_t k, uint_t c, unsigned shell ) { fusedStepShellPasses( r[k], &b[k], nullptr, nullptr, 0.0, c, level, shell ); } );
   }

   // ---- the steps of ChebyshevSmoother::solve (ChebyshevSmoother.hpp:165-212) on the three components, with the semantics of
   // P1ConstantOperator's (p1operator.hpp): one launch per step and cell on the inner points
   // (hyteg_hip_p1_elementwise_epsilon_chebyshev_*_macro_3d), the shell as in smooth_jac.  Where chebyshevFusable is false the
   // smoother runs its generic sequence.
   bool chebyshevFusable( uint_t level ) const { return fusedOn( level ); }
   // t = invDiag .* ( b - A x ); on the shell also x += c0 t.  On the inner points x is this launch's stencil source: its update
   // is carried out by the following chebyshevStep( ..., hasPrev = true ) or by chebyshevFinish
   void chebyshevStart( const dstType& t, const srcType& b, const srcType& x, double c0, uint_t level, const Selection& flagIn ) const
   {
      ScopedTimer timerOp( storage_->getTimingTree(), "Operator P1VectorFunction to P1VectorFunction" ), timerCheb( storage_->getTimingTree(), "chebyshev" );
      const auto& invDiag = *getInverseDiagonalValues();
      checkDistinct( "chebyshevStart", t, { &b, &x, &invDiag } );
      const auto flag = x.effectiveFlag( flagIn );
      sharesInnerShell(
          t, x, level, flag.data(),
          [&]( uint_t c, const double* cc, unsigned comps ) {
             double*       d[3];
             const double *f[3], *s[3], *i[3];
             cellPointers( t, c, level, d ), cellPointers( b, c, level, f ), cellPointers( x, c, level, s ), cellPointers( invDiag, c, level, i );
             hipCheck( hyteg_hip_p1_elementwise_epsilon_chebyshev_start_macro_3d( d, f, s, i, mu_.getCellPointer( c, level ), cc, int64_t( 1 ) << level,
                                                                                  comps, storage_->stream() ),
                       "P1ElementwiseAffineEpsilonOperator::chebyshevStart: cell" );
          },
          [&]( uint_t k, uint_t c, unsigned shell ) { fusedStepShellPasses( t[k], &b[k], &invDiag[k], &x[k], c0, c, level, shell ); } );
   }
   // tOut = invDiag .* ( A tIn ); x = ( x + cPrev tIn ) + cCur tOut on the inner points (first term only if hasPrev: the update
   // chebyshevStart left open), x += cCur tOut on the shell
   void chebyshevStep( const dstType& tOut, const dstType& x, const srcType& tIn, double cPrev, double cCur, bool hasPrev, uint_t level,
                       const Selection& flagIn ) const
   {
      ScopedTimer timerOp( storage_->getTimingTree(), "Operator P1VectorFunction to P1VectorFunction" ), timerCheb( storage_->getTimingTree(), "chebyshev" );
      const auto& invDiag = *getInverseDiagonalValues();
      checkDistinct( "chebyshevStep", tOut, { &x, &tIn, &invDiag } );
      checkDistinct( "chebyshevStep", x, { &tIn, &invDiag } );
      const auto flag = x.effectiveFlag( flagIn );
      sharesInnerShell(
          tOut, tIn, level, flag.data(),
          [&]( uint_t c, const double* cc, unsigned comps ) {
             double *      d[3], *u[3];
             const double *s[3], *i[3];
             cellPointers( tOut, c, level, d ), cellPointers( x, c, level, u ), cellPointers( tIn, c, level, s ), cellPointers( invDiag, c, level, i );
             hipCheck( hyteg_hip_p1_elementwise_epsilon_chebyshev_step_macro_3d( d, u, s, i, mu_.getCellPointer( c, level ), cc, int64_t( 1 ) << level,
                                                                                 cPrev, cCur, hasPrev ? 1 : 0, comps, storage_->stream() ),
                       "P1ElementwiseAffineEpsilonOperator::chebyshevStep: cell" );
          },
          [&]( uint_t k, uint_t c, unsigned shell ) { fusedStepShellPasses( tOut[k], nullptr, &invDiag[k], &x[k], cCur, c, level, shell ); } );
   }
   // x += c t on the inner points: closes a smoother call of order 1 (no step follows the start)
   void chebyshevFinish( const dstType& x, const srcType& t, double c, uint_t level, const Selection& flagIn ) const
   {
      const auto flag = x.effectiveFlag( flagIn );
      storage_->forLocalCells( [&]( uint_t ci, const MacroCell& cell ) {
         for ( uint_t k = 0; k < 3; ++k )
            chebyshevFinishCell( x[k], t[k], c, ci, level, storage_->maskFor( cell, flag[k] ) & HYTEG_HIP_MASK_INNER );
      } );
   }

 private:
   void checkDistinct( const char* who, const dstType& dst, std::initializer_list< const srcType* > inputs ) const
   {
      bool bad = false;
      for ( uint_t i = 0; i < 3; ++i )
      {
         bad = bad || &dst[i] == &mu_ || &dst[i] == &dst[( i + 1 ) % 3];
         for ( const srcType* f : inputs )
            for ( uint_t j = 0; j < 3; ++j )
               bad = bad || &dst[i] == &( *f )[j];
      }
      if ( bad )
         throw std::runtime_error( std::string( "P1ElementwiseAffineEpsilonOperator::" ) + who + ": dst must differ from its inputs and from mu" );
   }
   // the fused entries act on the inner points: below level 2 there are none, and setFused( false ) composes everywhere
   bool fusedOn( uint_t level ) const { return fused_ && level >= HYTEG_HIP_MIN_LEVEL; }
   template < class T >
   static void cellPointers( const srcType& f, uint_t c, uint_t level, T* ( &p )[3] )
   {
      for ( uint_t k = 0; k < 3; ++k )
         p[k] = f[k].getCellPointer( c, level );
   }
   // the schedule of a fused step out = f( A src ): this cell's shares of A src on the shell classes, the additive exchange of the
   // shares (the first overlaps the inner points) around inner( cell index, macro_vertex_coords, components whose inner points are
   // selected ), then shell( component, cell index, shell classes )
   template < class Inner, class Shell >
   void sharesInnerShell( const dstType& out, const srcType& src, uint_t level, const Selection flag[3], Inner&& inner, Shell&& shell ) const
   {
      const P1Function< double >* o[3] = { &out[0], &out[1], &out[2] };
      storage_->forLocalCells(
          [&]( uint_t c, const MacroCell& cell ) { kernel( o, src, c, cell, level, flag, HYTEG_HIP_MASK_SHELL, HYTEG_HIP_REPLACE ); } );
      out[0].beginSumSharedCopies( level, flag[0] );
      storage_->forLocalCells( [&]( uint_t c, const MacroCell& cell ) {
         unsigned comps = 0;
         for ( uint_t k = 0; k < 3; ++k )
            comps |= ( storage_->maskFor( cell, flag[k] ) & HYTEG_HIP_MASK_INNER ) ? ( 1u << k ) : 0u;
         if ( !comps || level < HYTEG_HIP_MIN_LEVEL )
            return;
         double cc[12];
         coordsOf( cell, cc );
         inner( c, cc, comps );
      } );
      out[0].endSumSharedCopies( level, flag[0] );
      for ( uint_t k = 1; k < 3; ++k )
         out[k].sumSharedCopies( level, flag[k] );
      storage_->forLocalCells( [&]( uint_t c, const MacroCell& cell ) {
         for ( uint_t k = 0; k < 3; ++k )
            shell( k, c, storage_->maskFor( cell, flag[k] ) & HYTEG_HIP_MASK_SHELL );
      } );
   }
   // one call for the classes of `classes` that the components' flags select on this cell
   void kernel( const P1Function< double >* const out[3], const srcType& src, uint_t c, const MacroCell& cell, uint_t level, const Selection flag[3],
                unsigned classes, int update ) const
   {
      unsigned masks[3];
      for ( uint_t k = 0; k < 3; ++k )
         masks[k] = storage_->maskFor( cell, flag[k] ) & classes;
      if ( ( masks[0] | masks[1] | masks[2] ) == 0 )
         return;
      double cc[12];
      coordsOf( cell, cc );
      double*       d[3] = { out[0]->getCellPointer( c, level ), out[1]->getCellPointer( c, level ), out[2]->getCellPointer( c, level ) };
      const double* s[3] = { src[0].getCellPointer( c, level ), src[1].getCellPointer( c, level ), src[2].getCellPointer( c, level ) };
      hipCheck( hyteg_hip_p1_elementwise_epsilon_apply_macro_3d_component_masks( d, s, mu_.getCellPointer( c, level ), cc, int64_t( 1 ) << level, masks,
                                                                                 update, storage_->stream() ),
                "P1ElementwiseAffineEpsilonOperator::apply: cell" );
   }

   std::shared_ptr< PrimitiveStorage >           storage_;
   uint_t                                        minLevel_, maxLevel_;
   const P1Function< double >&                   mu_;
   uint64_t                                      uid_   = nextUid();
   bool                                          fused_ = true;
   std::shared_ptr< P1VectorFunction< double > > invDiag_;
};

// P1P1ElementwiseAffineEpsilonStokesOperator.hpp:32-92: the epsilon operator on the velocity, the constant-stencil div / divT blocks
// and the PSPG block of P1P1StokesOperator
class P1P1ElementwiseAffineEpsilonStokesOperator
{
 public:
   using srcType            = P1StokesFunction< double >;
   using dstType            = srcType;
   using VelocityOperator_T = P1ElementwiseAffineEpsilonOperator;
   static constexpr bool hasPspgBlock = true; // has_pspg_block, P1P1ElementwiseAffineEpsilonStokesOperator.hpp:86-90

   P1P1ElementwiseAffineEpsilonStokesOperator( const std::shared_ptr< PrimitiveStorage >& storage, uint_t minLevel, uint_t maxLevel,
                                               const P1Function< double >& mu )
   : viscOp( storage, minLevel, maxLevel, mu )
   , div( storage, minLevel, maxLevel )
   , divT( storage, minLevel, maxLevel )
   , pspg( storage, minLevel, maxLevel )
   , storage_( storage )
   {}

   // lines 57-69
   void apply( const srcType& src, const dstType& dst, uint_t level, DoFType flag, UpdateType = Replace ) const
   {
      if ( &src == &dst )
         throw std::runtime_error( "P1P1ElementwiseAffineEpsilonStokesOperator::apply: src and dst must differ" );
      viscOp.apply( src.uvw(), dst.uvw(), level, flag, Replace );
      divT.apply( src.p(), dst.uvw(), level, flag, Add );
      div.apply( src.uvw(), dst.p(), level, flag, Replace );
      pspg.apply( src.p(), dst.p(), level, flag, Add );
   }
   const VelocityOperator_T&           getA() const { return viscOp; }
   std::shared_ptr< PrimitiveStorage > getStorage() const { return storage_; }
   uint64_t                            uid() const { return uid_; }

   P1ElementwiseAffineEpsilonOperator viscOp;
   P1ConstantDivOperator              div;
   P1ConstantDivTOperator             divT;
   P1PSPGOperator                     pspg;

 private:
   std::shared_ptr< PrimitiveStorage > storage_;
   uint64_t                            uid_ = nextUid();
};

// dst = mu .* invLumpedMass .* src pointwise: nodal quadrature of the 1 / mu - weighted lumped mass matrix (the direction of the
// reference's commented-out varViscStokesMinResSolver, src/hyteg/solvers/solvertemplates/StokesSolverTemplates.hpp).  The pressure
// action of the viscosity-weighted preconditioners; the product is formed once, at construction.
class P1ViscosityWeightedLumpedInvMassOperator
{
 public:
   P1ViscosityWeightedLumpedInvMassOperator( const std::shared_ptr< PrimitiveStorage >& storage, uint_t minLevel, uint_t maxLevel,
                                             const P1Function< double >& mu )
   : scale_( "viscosity_weighted_lumped_inv_mass", storage, minLevel, maxLevel )
   , tmp_( "viscosity_weighted_lumped_inv_mass_tmp", storage, minLevel, maxLevel )
   {
      scale_.setBoundaryConditionAllInner();
      tmp_.setBoundaryConditionAllInner();
      P1LumpedInvMassOperator lumped( storage, minLevel, maxLevel );
      for ( uint_t l = minLevel; l <= maxLevel; ++l )
         scale_.multElementwise( { mu, lumped.getInverseLumpedMass() }, l, All );
   }
   void apply( const P1Function< double >& src, const P1Function< double >& dst, uint_t level, DoFType flag, UpdateType updateType = Replace ) const
   {
      applyPointwiseScaling( scale_, tmp_, src, dst, level, flag, updateType );
   }

 private:
   P1Function< double > scale_, tmp_;
};

// StokesPressureBlockPreconditioner with the pressure action above
template < class OperatorType >
class StokesViscosityWeightedPressureBlockPreconditioner : public Solver< OperatorType >
{
 public:
   using FunctionType = typename OperatorType::srcType;
   StokesViscosityWeightedPressureBlockPreconditioner( const std::shared_ptr< PrimitiveStorage >& storage, uint_t minLevel, uint_t maxLevel,
                                                       const P1Function< double >& mu )
   : pressure_( storage, minLevel, maxLevel, mu )
   , flag_( Inner | NeumannBoundary | FreeslipBoundary )
   {}
   void solve( const OperatorType&, const FunctionType& x, const FunctionType& b, uint_t level ) override
   {
      x.assign( { 1.0 }, { b }, level, flag_ );
      pressure_.apply( b.p(), x.p(), level, flag_, Replace );
   }

 private:
   P1ViscosityWeightedLumpedInvMassOperator pressure_;
   DoFType                                  flag_;
};

} // namespace hyteg
