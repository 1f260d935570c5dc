// p2epsilon.hpp -- part of the C++ host layer above the C-ABI (see hyteg_host.hpp for the data model).
// Variable-viscosity Stokes on P2-P1 (Taylor-Hood):
//   operatorgeneration::P2ViscousBlockEpsilonOperator( storage, minLevel, maxLevel, const P2Function< real_t >& mu )
//   operatorgeneration::P2P1StokesEpsilonOperator( storage, minLevel, maxLevel, mu )
// of module hyteg_operators: the operators the reference's convection apps instantiate.  Their mu = 1 case is the in-tree
// P2ElementwiseAffineEpsilonOperator / P2P1ElementwiseAffineEpsilonStokesOperator (src/mixed_operator/
// P2P1ElementwiseAffineEpsilonStokesOperator.hpp:33-88, apply :61-70), the P2 half of
// tests/hyteg/convergence/ElementwiseEpsilonMinResConvergenceTest.cpp:156-163, 366-412.  The viscosity is a P2Function that the caller
// interpolates on every level used (the operator at level l reads mu at level l), as the coefficient of P2ElementwiseDivKGrad.
// The reference composes the velocity block of nine P2 elementwise blocks; here one C-ABI call per macro-cell computes the three
// components (hyteg_hip_p2_elementwise_epsilon_apply_cell_kinds) with the schedule of P2ElementwiseDivKGrad::gemv: every cell adds the
// contributions of its own micro-cells, the additive exchange completes the shared DoFs.  No smooth_sor.  The operator offers what
// GeometricMultigridSolver and ChebyshevSmoother look for (residual, chebyshevStart / Step / Finish) and a fused smooth_jac: one launch
// per step and cell for the three components (hyteg_hip_p2_elementwise_epsilon_*_cell, schedule: p2varcoefsteps.hpp).
#pragma once

#include "p1epsilon.hpp"
#include "p2divkgrad.hpp"
#include "taylorhood.hpp"

namespace hyteg {

// P2toP2QuadraticVectorRestriction.hpp / P2toP2QuadraticVectorProlongation.hpp: the quadratic P2 transfer on every component of a
// P2VectorFunction (the grid transfer of a multigrid cycle on P2ViscousBlockEpsilonOperator)
using P2toP2QuadraticVectorRestriction  = VectorFunctionRestriction< P2toP2QuadraticRestriction >;
using P2toP2QuadraticVectorProlongation = VectorFunctionProlongation< P2toP2QuadraticProlongation >;

namespace operatorgeneration {

class P2ViscousBlockEpsilonOperator
{
 public:
   using srcType = P2VectorFunction< double >;
   using dstType = P2VectorFunction< double >;

   P2ViscousBlockEpsilonOperator( const std::shared_ptr< PrimitiveStorage >& storage, uint_t minLevel, uint_t maxLevel, const P2Function< double >& mu )
   : storage_( storage )
   , minLevel_( minLevel )
   , maxLevel_( maxLevel )
   , mu_( mu )
   {
      if ( (int) maxLevel > hyteg_hip_p2_elementwise_epsilon_max_level() )
         throw std::runtime_error( "P2ViscousBlockEpsilonOperator: levels 0..8" );
      storage->markInUse(); // the mesh boundary flags are fixed from here on
      for ( uint_t l = minLevel; l <= maxLevel; ++l )
         for ( uint_t lc = 0; lc < storage->getNumberOfLocalCells(); ++lc )
         {
            double                   cc[12];
            std::array< double, 72 > g;
            coordsOf( storage->getLocalCell( lc ), cc );
            hipCheck( hyteg_hip_p2_elementwise_epsilon_geometry( cc, (int) l, g.data() ), "P2ViscousBlockEpsilonOperator: geometry" );
            geometry_[l].push_back( g );
         }
   }
   std::shared_ptr< PrimitiveStorage > getStorage() const { return storage_; }
   uint_t                              getMinLevel() const { return minLevel_; }
   uint_t                              getMaxLevel() const { return maxLevel_; }
   const P2Function< double >&         getViscosity() const { return mu_; }
   uint64_t                            uid() const { return uid_; }

   // the fused Jacobi, residual and Chebyshev entries (default), or the composed passes everywhere (tests, measurements)
   void setFused( bool on ) { fused_ = on; }
   bool getFused() const { return fused_; }

   // Operator::apply = gemv( 1, src, updateType == Replace ? 0 : 1, dst )
   void apply( const srcType& src, const dstType& dst, uint_t level, const Selection& flag, UpdateType updateType = Replace ) const
   {
      gemv( 1.0, src, updateType == Replace ? 0.0 : 1.0, dst, level, flag );
   }
   // the schedule of P2ElementwiseDivKGrad::gemv on the three components in one pass.  Every component has its own boundary condition
   // (VectorToVectorOperator applies block ( i, j ) with the flag on dst[i]): the kernels take a class mask per component
   void gemv( double alpha, const srcType& src, double beta, const dstType& dst, uint_t level, const Selection& flagIn ) const
   {
      checkDistinct( "gemv", dst, src );
      const std::array< Selection, 3 > flag   = dst.effectiveFlag( flagIn );
      const bool                       shared = storage_->getCells().size() > 1;
      if ( !shared )
      {
         if ( beta != 0.0 && beta != 1.0 )
            for ( uint_t k = 0; k < 3; ++k )
               dst[k].assign( { beta }, { dst[k] }, level, flag[k] );
         launch( alpha, src, dst, level, flag, beta == 0.0 ? HYTEG_HIP_REPLACE : HYTEG_HIP_ADD );
         return;
      }
      if ( beta == 0.0 )
      {
         launch( alpha, src, dst, level, flag, HYTEG_HIP_REPLACE );
         sumShared( dst, level, flag );
         return;
      }
      P2VectorFunction< double > tmp( "p2_epsilon_gemv_tmp", storage_, level, level );
      launch( alpha, src, tmp, level, flag, HYTEG_HIP_REPLACE );
      sumShared( tmp, level, flag );
      for ( uint_t k = 0; k < 3; ++k )
         dst[k].assign( { beta, 1.0 }, { dst[k], tmp[k] }, level, flag[k] );
   }

   // VectorToVectorOperator::computeInverseDiagonalOperatorValues + extractInverseDiagonal: the inverse diagonals of the three diagonal
   // blocks.  Per cell the diagonal kernel, the additive exchange, and the reciprocal on the host (set-up time, once per operator)
   void computeInverseDiagonalOperatorValues()
   {
      invDiag_.reset( new P2VectorFunction< double >( "inverse diagonal entries", storage_, minLevel_, maxLevel_ ) );
      const P2VectorFunction< double >& d = *invDiag_;
      for ( uint_t l = minLevel_; l <= maxLevel_; ++l )
      {
         for ( uint_t c = 0; c < storage_->getNumberOfLocalCells(); ++c )
         {
            double* dv[3];
            double* de[3];
            for ( uint_t k = 0; k < 3; ++k )
               dv[k] = d[k].getVertexDoFFunction().getCellPointer( c, l ), de[k] = d[k].getEdgeCellPointer( c, l );
            hipCheck( hyteg_hip_p2_elementwise_epsilon_diagonal_cell( dv, de, mu_.getVertexDoFFunction().getCellPointer( c, l ), mu_.getEdgeCellPointer( c, l ),
                                                                      (int) l, geometry_.at( l ).at( c ).data(), storage_->stream() ),
                      "P2ViscousBlockEpsilonOperator: diagonal" );
         }
         for ( uint_t k = 0; k < 3; ++k )
         {
            if ( storage_->getCells().size() > 1 )
            {
               d[k].getVertexDoFFunction().sumSharedCopies( l, All );
               d[k].sumSharedEdgeCopies( l, All );
            }
            invertElementwise( d[k], l );
         }
      }
   }
   bool                                          hasInverseDiagonalValues() const { return invDiag_ != nullptr; }
   std::shared_ptr< P2VectorFunction< double > > getInverseDiagonalValues() const
   {
      if ( !invDiag_ )
         throw std::runtime_error( "Inverse diagonal values have not been assembled, call computeInverseDiagonalOperatorValues() "
                                   "to set up this function." );
      return invDiag_;
   }

   // P2ElementwiseOperator::smooth_jac (P2ElementwiseOperator.cpp:344-374) on the three components, statement by statement:
   //   dst = A src;  dst = rhs - dst;  dst = D^-1 dst;  dst = src + relax dst
   // Fused: the four statements in the epilogue of the apply kernels (hyteg_hip_p2_elementwise_epsilon_jacobi_cell); components with
   // different boundary conditions stay on this path (a class mask per component)
   void smooth_jac( const dstType& dst, const srcType& rhs, const srcType& src, double relax, uint_t level, const Selection& flag ) const
   {
      const auto& invDiag = *getInverseDiagonalValues();
      if ( fused_ && !sharesComponent( dst, { &rhs, &invDiag } ) )
      {
         checkDistinct( "smooth_jac", dst, src );
         step( p2varcoef::Step::Jacobi, dst, &src, &rhs, &invDiag, nullptr, dst.effectiveFlag( flag ), level, relax, 0.0, false );
         return;
      }
      apply( src, dst, level, flag );
      for ( uint_t k = 0; k < 3; ++k )
      {
         dst[k].assign( { 1.0, -1.0 }, { rhs[k], dst[k] }, level, flag );
         dst[k].multElementwise( { invDiag[k], dst[k] }, level, flag );
         dst[k].assign( { 1.0, relax }, { src[k], dst[k] }, level, flag );
      }
   }

   // r = b - A x as the multigrid cycle writes it (GeometricMultigridSolver.hpp:240-246: apply, then assign, over three components).
   // Fused: one launch per cell (hyteg_hip_p2_elementwise_epsilon_residual_cell); composed where r shares a component with x or b, and with
   // setFused( false )
   void residual( const srcType& x, const srcType& b, const dstType& r, uint_t level, const Selection& flag ) const
   {
      if ( !fused_ || sharesComponent( r, { &x, &b } ) )
      {
         apply( x, r, level, flag );
         for ( uint_t k = 0; k < 3; ++k )
            r[k].assign( { 1.0, -1.0 }, { b[k], r[k] }, level, flag );
         return;
      }
      checkDistinct( "residual", r, x );
      step( p2varcoef::Step::Residual, r, &x, &b, nullptr, nullptr, r.effectiveFlag( flag ), level, 0.0, 0.0, false );
   }

   // ---- the steps of ChebyshevSmoother::solve (ChebyshevSmoother.hpp:165-212) on the three components, with the semantics of
   // P1ConstantOperator's (p1operator.hpp): one launch per step and cell (hyteg_hip_p2_elementwise_epsilon_chebyshev_*_cell).  Where
   // chebyshevFusable is false the smoother runs its generic sequence.
   bool chebyshevFusable( uint_t ) const { return fused_; }
   // t = invDiag .* ( b - A x ); on the shell of several cells also x += c0 t.  Elsewhere x is this launch's source: its update is carried
   // out by the following chebyshevStep( ..., hasPrev = true ) or by chebyshevFinish
   void chebyshevStart( const dstType& t, const srcType& b, const srcType& x, double c0, uint_t level, const Selection& flag ) const
   {
      const auto& invDiag = *getInverseDiagonalValues();
      checkOutput( "chebyshevStart", t, { &b, &x, &invDiag } );
      step( p2varcoef::Step::ChebStart, t, &x, &b, &invDiag, &x, x.effectiveFlag( flag ), level, c0, 0.0, false );
   }
   // tOut = invDiag .* ( A tIn ); x = ( x + cPrev tIn ) + cCur tOut (first term only if hasPrev: the update chebyshevStart left open); on the
   // shell of several cells x += cCur tOut
   void chebyshevStep( const dstType& tOut, const dstType& x, const srcType& tIn, double cPrev, double cCur, bool hasPrev, uint_t level,
                       const Selection& flag ) const
   {
      const auto& invDiag = *getInverseDiagonalValues();
      checkOutput( "chebyshevStep", tOut, { &x, &tIn, &invDiag } );
      checkOutput( "chebyshevStep", x, { &tIn, &invDiag } );
      step( p2varcoef::Step::ChebStep, tOut, &tIn, nullptr, &invDiag, &x, x.effectiveFlag( flag ), level, cCur, cPrev, hasPrev );
   }
   // x += c t where the start deferred it: closes a smoother call of order 1 (no step follows the start)
   void chebyshevFinish( const dstType& x, const srcType& t, double c, uint_t level, const Selection& flag ) const
   {
      p2varcoef::chebyshevFinish< 3 >( storage_, { &x[0], &x[1], &x[2] }, { &t[0], &t[1], &t[2] }, x.effectiveFlag( flag ), c, level );
   }

 private:
   // does a component of out belong to one of the functions as well?
   static bool sharesComponent( const dstType& out, std::initializer_list< const srcType* > functions )
   {
      for ( const srcType* f : functions )
         for ( uint_t i = 0; i < 3; ++i )
            for ( uint_t j = 0; j < 3; ++j )
               if ( &out[i] == &( *f )[j] )
                  return true;
      return false;
   }
   void checkOutput( const char* who, const dstType& out, std::initializer_list< const srcType* > inputs ) const
   {
      bool bad = sharesComponent( out, inputs );
      for ( uint_t i = 0; i < 3; ++i )
         bad = bad || &out[i] == &mu_ || &out[i] == &out[( i + 1 ) % 3];
      if ( bad )
         throw std::runtime_error( std::string( "P2ViscousBlockEpsilonOperator::" ) + who + ": an output must differ from the inputs and from mu" );
   }
   template < class T >
   static void cellPointers( const std::array< const P2Function< double >*, 3 >& g, uint_t c, uint_t level, T* ( &v )[3], T* ( &e )[3] )
   {
      for ( uint_t k = 0; k < 3; ++k )
         v[k] = g[k] ? g[k]->getVertexDoFFunction().getCellPointer( c, level ) : nullptr, e[k] = g[k] ? g[k]->getEdgeCellPointer( c, level ) : nullptr;
   }
   // one fused step (p2varcoefsteps.hpp): a = relax, c0 or cCur; a function the step does not have is null
   void step( p2varcoef::Step what, const dstType& out, const srcType* src, const srcType* rhs, const srcType* inv, const dstType* x,
              const std::array< Selection, 3 >& flag, uint_t level, double a, double cPrev, bool hasPrev ) const
   {
      const auto comps = []( const srcType* f ) {
         return f ? std::array< const P2Function< double >*, 3 >{ &( *f )[0], &( *f )[1], &( *f )[2] } :
                    std::array< const P2Function< double >*, 3 >{ nullptr, nullptr, nullptr };
      };
      const p2varcoef::Operands< 3 > f{ comps( &out ), comps( src ), comps( rhs ), comps( inv ), comps( x ) };
      p2varcoef::fusedStep< 3 >(
          storage_, what, f, flag, level, a, [&] { launch( 1.0, *src, out, level, flag, HYTEG_HIP_REPLACE, HYTEG_HIP_MASK_SHELL ); },
          [&]( uint_t c, const std::array< unsigned, 3 >& m ) {
             double *ov[3], *oe[3], *xv[3], *xe[3];
             const double *sv[3], *se[3], *rv[3], *re[3], *iv[3], *ie[3];
             cellPointers( f.out, c, level, ov, oe ), cellPointers( f.src, c, level, sv, se ), cellPointers( f.rhs, c, level, rv, re );
             cellPointers( f.inv, c, level, iv, ie ), cellPointers( f.x, c, level, xv, xe );
             const double *           mv = mu_.getVertexDoFFunction().getCellPointer( c, level ), *me = mu_.getEdgeCellPointer( c, level );
             const double*            geo = geometry_.at( level ).at( c ).data();
             const int                l   = (int) level;
             const hyteg_hip_stream_t s   = storage_->stream();
             int                      rc  = 0;
             switch ( what )
             {
             case p2varcoef::Step::Residual:
                rc = hyteg_hip_p2_elementwise_epsilon_residual_cell( ov, oe, sv, se, rv, re, mv, me, m.data(), l, geo, 0xFFu, s );
                break;
             case p2varcoef::Step::Jacobi:
                rc = hyteg_hip_p2_elementwise_epsilon_jacobi_cell( ov, oe, sv, se, rv, re, iv, ie, mv, me, m.data(), l, geo, a, 0xFFu, s );
                break;
             case p2varcoef::Step::ChebStart:
                rc = hyteg_hip_p2_elementwise_epsilon_chebyshev_start_cell( ov, oe, sv, se, rv, re, iv, ie, mv, me, m.data(), l, geo, 0xFFu, s );
                break;
             case p2varcoef::Step::ChebStep:
                rc = hyteg_hip_p2_elementwise_epsilon_chebyshev_step_cell( ov, oe, xv, xe, sv, se, iv, ie, mv, me, m.data(), l, geo, cPrev, a, hasPrev ? 1 : 0,
                                                                           0xFFu, s );
                break;
             }
             hipCheck( rc, "P2ViscousBlockEpsilonOperator: fused step" );
          } );
   }
   // views of the same functions are different VectorFunction objects (the C facade builds one per argument): compare components
   void checkDistinct( const char* who, const dstType& dst, const srcType& src ) const
   {
      bool bad = false;
      for ( uint_t i = 0; i < 3; ++i )
      {
         bad = bad || &dst[i] == &mu_ || &dst[i] == &dst[( i + 1 ) % 3];
         for ( uint_t j = 0; j < 3; ++j )
            bad = bad || &dst[i] == &src[j];
      }
      if ( bad )
         throw std::runtime_error( std::string( "P2ViscousBlockEpsilonOperator::" ) + who + ": dst must differ from src and from mu" );
   }
   void sumShared( const dstType& f, uint_t level, const std::array< Selection, 3 >& flag ) const
   {
      for ( uint_t k = 0; k < 3; ++k )
      {
         f[k].getVertexDoFFunction().sumSharedCopies( level, flag[k] );
         f[k].sumSharedEdgeCopies( level, flag[k] );
      }
   }
   void launch( double alpha, const srcType& src, const dstType& dst, uint_t level, const std::array< Selection, 3 >& flag, int update,
                unsigned keep = HYTEG_HIP_MASK_ALL ) const
   {
      const std::vector< unsigned > masks[3] = { storage_->masksFor( flag[0], false, keep ), storage_->masksFor( flag[1], false, keep ),
                                                 storage_->masksFor( flag[2], false, keep ) };
      for ( uint_t c = 0; c < storage_->getNumberOfLocalCells(); ++c )
      {
         double *       dv[3], *de[3];
         const double * sv[3], *se[3];
         const unsigned m[3] = { masks[0][c], masks[1][c], masks[2][c] };
         for ( uint_t k = 0; k < 3; ++k )
         {
            dv[k] = dst[k].getVertexDoFFunction().getCellPointer( c, level ), de[k] = dst[k].getEdgeCellPointer( c, level );
            sv[k] = src[k].getVertexDoFFunction().getCellPointer( c, level ), se[k] = src[k].getEdgeCellPointer( c, level );
         }
         hipCheck( hyteg_hip_p2_elementwise_epsilon_apply_cell_kinds( dv, de, sv, se, mu_.getVertexDoFFunction().getCellPointer( c, level ),
                                                                      mu_.getEdgeCellPointer( c, level ), m, (int) level,
                                                                      geometry_.at( level ).at( c ).data(), alpha, update, 0xFFu, storage_->stream() ),
                   "P2ViscousBlockEpsilonOperator::gemv" );
      }
   }

   std::shared_ptr< PrimitiveStorage >                         storage_;
   uint_t                                                      minLevel_, maxLevel_;
   const P2Function< double >&                                 mu_;
   std::map< uint_t, std::vector< std::array< double, 72 > > > geometry_; // per level and local cell
   uint64_t                                                    uid_ = nextUid();
   std::shared_ptr< P2VectorFunction< double > >               invDiag_;
   bool                                                        fused_ = true;
};

// P2P1ElementwiseAffineEpsilonStokesOperator.hpp:61-70: viscOp Replace, divT Add, div Replace; no stabilisation block.  The mixed blocks
// are those of P2P1TaylorHoodStokesOperator (taylorhood.hpp); StokesOperator (stokes.hpp) builds its velocity block from a scalar
// operator without a coefficient, so the composition is written out here, as P1P1ElementwiseAffineEpsilonStokesOperator is.
class P2P1StokesEpsilonOperator
{
 public:
   using srcType            = P2P1TaylorHoodFunction< double >;
   using dstType            = srcType;
   using VelocityOperator_T = P2ViscousBlockEpsilonOperator;
   static constexpr bool hasPspgBlock = false;

   P2P1StokesEpsilonOperator( const std::shared_ptr< PrimitiveStorage >& storage, uint_t minLevel, uint_t maxLevel, const P2Function< double >& mu )
   : viscOp( storage, minLevel, maxLevel, mu )
   , div( storage, minLevel, maxLevel )
   , divT( storage, minLevel, maxLevel )
   , storage_( storage )
   {}

   void apply( const srcType& src, const dstType& dst, uint_t level, DoFType flag, UpdateType = Replace ) const
   {
      if ( &src == &dst )
         throw std::runtime_error( "P2P1StokesEpsilonOperator::apply: src and dst must differ" );
      viscOp.apply( src.uvw(), dst.uvw(), level, flag, Replace );
      divT.apply( src.p(), dst.uvw(), level, flag, Add );
      div.apply( src.uvw(), dst.p(), level, flag, Replace );
   }
   const VelocityOperator_T&           getA() const { return viscOp; }
   std::shared_ptr< PrimitiveStorage > getStorage() const { return storage_; }
   uint64_t                            uid() const { return uid_; }

   P2ViscousBlockEpsilonOperator viscOp;
   P2ToP1DivOperator             div;
   P1ToP2DivTOperator            divT;

 private:
   std::shared_ptr< PrimitiveStorage > storage_;
   uint64_t                            uid_ = nextUid();
};

} // namespace operatorgeneration
} // namespace hyteg
