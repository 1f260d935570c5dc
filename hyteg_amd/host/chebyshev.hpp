// chebyshev.hpp -- part of the C++ host layer above the C-ABI (see hyteg_host.hpp for the data model).
// ChebyshevSmoother< OperatorType >, chebyshev::estimateRadius, InvDiagOperatorWrapper< OperatorType >
// (src/hyteg/solvers/ChebyshevSmoother.hpp, src/hyteg/numerictools/SpectrumEstimation.hpp:56-84)
//
// Out of scope: projection operators, substitute preconditioners (setPreconditioner) and lowMemoryMode.
#pragma once

#include <cmath>

#include "solvers.hpp"

namespace hyteg {

namespace chebyshev {

// the monomial form loses about half a digit per order (the coefficients alternate in sign and grow like ( 2 / delta )^order):
// orders 1-5 reproduce the defining polynomial on [0, upper] to 3e-14, order 8 to 8e-13 (bounds 0.3 rho / 1.2 rho, 0.1 / 1, 0.5 / 4);
// higher orders are rejected -- stack smoother calls instead
constexpr uint_t kMaxOrder = 8;

// Coefficients c[0 .. order-1] of p( lambda ) = sum_k c[k] lambda^k in
//      1 - lambda p( lambda ) = T_n( ( theta - lambda ) / delta ) / T_n( theta / delta ),   theta = ( upper + lower ) / 2,
//                                                                                           delta = ( upper - lower ) / 2
// -- what ChebyshevSmoother::setupCoefficientsInternal (ChebyshevSmoother.hpp:329-552) tabulates in closed form for orders 1-5.
// Here, for any order: U_k( lambda ) = delta^k T_k( ( theta - lambda ) / delta ) obeys
//      U_0 = 1,  U_1 = theta - lambda,  U_{k+1} = 2 ( theta - lambda ) U_k - delta^2 U_{k-1}
// (the Chebyshev recurrence times delta^{k+1}); carried out on monomial coefficients in extended precision, then
// c[k] = - u_{k+1} / u_0 with U_n = sum_j u_j lambda^j.  Touches no GPU.
inline std::vector< double > coefficients( uint_t order, double lowerBound, double upperBound )
{
   if ( order < 1 || order > kMaxOrder )
      throw std::runtime_error( "chebyshev::coefficients: order must be in [1, " + std::to_string( kMaxOrder ) + "]" );
   if ( !( lowerBound > 0.0 ) || !( upperBound > lowerBound ) )
      throw std::runtime_error( "chebyshev::coefficients: need 0 < lowerBound < upperBound" );
   using real = long double;
   const real theta = 0.5L * ( (real) upperBound + (real) lowerBound );
   const real delta = 0.5L * ( (real) upperBound - (real) lowerBound );
   std::vector< real > prev{ 1.0L }, cur{ theta, -1.0L };
   for ( uint_t k = 1; k < order; ++k )
   {
      std::vector< real > next( cur.size() + 1, 0.0L );
      for ( size_t j = 0; j < cur.size(); ++j )
      {
         next[j] += 2.0L * theta * cur[j];
         next[j + 1] -= 2.0L * cur[j];
      }
      for ( size_t j = 0; j < prev.size(); ++j )
         next[j] -= delta * delta * prev[j];
      prev = std::move( cur );
      cur  = std::move( next );
   }
   std::vector< double > c( order );
   for ( uint_t k = 0; k < order; ++k )
      c[k] = (double) ( -cur[k + 1] / cur[0] );
   return c;
}

} // namespace chebyshev

// dst = invDiag .* ( A src ): the operator whose spectral radius bounds the Chebyshev polynomial
// (chebyshev::InvDiagOperatorWrapper, ChebyshevSmoother.hpp:562-640)
template < class OperatorType >
class InvDiagOperatorWrapper
{
 public:
   using srcType = typename OperatorType::srcType;
   using dstType = typename OperatorType::dstType;
   explicit InvDiagOperatorWrapper( const OperatorType& A )
   : A_( A )
   {}
   void apply( const srcType& src, const dstType& dst, uint_t level, const Selection& flag, UpdateType updateType = Replace ) const
   {
      if ( updateType != Replace )
         throw std::runtime_error( "InvDiagOperatorWrapper::apply: Replace only" );
      A_.apply( src, dst, level, flag );
      dst.multElementwise( { *A_.getInverseDiagonalValues(), dst }, level, flag );
   }

 private:
   const OperatorType& A_;
};

namespace chebyshev {

// chebyshev::estimateRadius (ChebyshevSmoother.hpp:655-666) = estimateSpectralRadiusWithPowerIteration on D^-1 A
// (SpectrumEstimation.hpp:56-84), statement by statement: normalise x, apply, then per iteration norm, scale, apply,
// radius = < x, D^-1 A x >, all with the flag All like the reference.  The inverse diagonals of this project's operators are
// assembled on every point (P1ConstantOperator::computeInverseDiagonalOperatorValues sets the sum of the neighbour cells'
// centre weights on all 14 boundary slots, fixed ones included; the elementwise operators sum element diagonals everywhere), so
// `All` is usable as it stands; every function reads it under its own boundary condition (effectiveFlag).
// x: start vector (overwritten), tmp: work function.  Reads the dot products back on the host: not for recorded cycles.
template < class OperatorType >
double estimateRadius( const OperatorType& A, uint_t level, uint_t maxIter, const std::shared_ptr< PrimitiveStorage >&,
                       const typename OperatorType::srcType& x, const typename OperatorType::srcType& tmp )
{
   InvDiagOperatorWrapper< OperatorType > op( A );
   double                                 norm = std::sqrt( x.dotGlobal( x, level, All ) );
   x.assign( { 1.0 / norm }, { x }, level, All );
   op.apply( x, tmp, level, All );
   double radius = 0.0;
   for ( uint_t it = 1; it <= maxIter; ++it )
   {
      norm = std::sqrt( tmp.dotGlobal( tmp, level, All ) );
      x.assign( { 1.0 / norm }, { tmp }, level, All );
      op.apply( x, tmp, level, All );
      radius = x.dotGlobal( tmp, level, All );
   }
   return radius;
}

} // namespace chebyshev

// does the operator offer the fused Chebyshev steps (P1ConstantOperator::chebyshevStart / chebyshevStep / chebyshevFinish)?
template < class OperatorType, class FunctionType, class = void >
struct HasChebyshevSteps : std::false_type
{};
template < class OperatorType, class FunctionType >
struct HasChebyshevSteps< OperatorType, FunctionType,
                          std::void_t< decltype( std::declval< const OperatorType& >().chebyshevStep(
                              std::declval< const FunctionType& >(), std::declval< const FunctionType& >(), std::declval< const FunctionType& >(), 0.0, 0.0,
                              false, uint_t( 0 ), All ) ) > > : std::true_type
{};

// ChebyshevSmoother.hpp:40-555.  One call of order n applies  x += p( D^-1 A ) D^-1 ( b - A x )  with the polynomial of
// chebyshev::coefficients by the reference's sequence
//      t2 = b - A x;  t1 = D^-1 t2;  x += c[0] t1;      for k = 1 .. n-1:  t2 = A t1;  t1 = D^-1 t2;  x += c[k] t1
// on Inner | NeumannBoundary | FreeslipBoundary.  The reference zeroes t1 before every D^-1 step; that only matters for the
// points the flag does not select (t1 is the next apply's source): here both temporaries are zero since their allocation
// and no step writes such a point (they are zeroed again if a call selects different points than the one before).
//  * generic path: apply, multElementwise, assign of any operator with getInverseDiagonalValues();
//  * fused path (setFused, default on; operators with chebyshevStart / chebyshevStep, levels the operator does not batch):
//    one launch per step on the cell interiors -- the update x += c[k-1] t of step k-1 is carried out by the launch of step k,
//    because x is the stencil source of the first launch (hyteg_hip_p1_chebyshev_{start,step}_cell).
// solve() allocates nothing, never synchronises and reads nothing back: a multigrid cycle with this smoother can be recorded.
template < class OperatorType >
class ChebyshevSmoother : public Solver< OperatorType >
{
 public:
   using FunctionType = typename OperatorType::srcType;

   ChebyshevSmoother( const std::shared_ptr< PrimitiveStorage >& storage, uint_t minLevel, uint_t maxLevel )
   : flag_( Inner | NeumannBoundary | FreeslipBoundary )
   , minLevel_( minLevel )
   , maxLevel_( maxLevel )
   , tmp1_( "cheb_tmp1", storage, minLevel, maxLevel )
   , tmp2_( "cheb_tmp2", storage, minLevel, maxLevel )
   , coefficients_( maxLevel - minLevel + 1 )
   , lastSelection_( maxLevel - minLevel + 1 )
   {}

   void setupCoefficients( uint_t order, const std::vector< double >& spectralRadii, double upperFactor = 1.2, double lowerFactor = 0.3 )
   {
      if ( spectralRadii.size() != maxLevel_ - minLevel_ + 1 )
         throw std::runtime_error( "ChebyshevSmoother::setupCoefficients: one spectral radius per level is needed" );
      for ( uint_t level = minLevel_; level <= maxLevel_; ++level )
         setupCoefficientsOnLevel( order, spectralRadii[level - minLevel_], level, upperFactor, lowerFactor );
   }
   void setupCoefficients( uint_t order, double spectralRadius, double upperFactor = 1.2, double lowerFactor = 0.3 )
   {
      for ( uint_t level = minLevel_; level <= maxLevel_; ++level )
         setupCoefficientsOnLevel( order, spectralRadius, level, upperFactor, lowerFactor );
   }
   void setupCoefficientsOnLevel( uint_t order, double spectralRadius, uint_t level, double upperFactor = 1.2, double lowerFactor = 0.3 )
   {
      setupCoefficientsInternal( order, lowerFactor * spectralRadius, upperFactor * spectralRadius, level );
   }
   void setupCoefficientsInternal( uint_t order, double lowerBound, double upperBound, uint_t level )
   {
      checkLevel( level );
      coefficients_[level - minLevel_] = chebyshev::coefficients( order, lowerBound, upperBound );
   }
   const std::vector< double >& getCoefficients( uint_t level ) const
   {
      checkLevel( level );
      return coefficients_[level - minLevel_];
   }

   // the fused steps where the operator has them (default), or the generic sequence everywhere (tests, measurements)
   void setFused( bool on ) { fused_ = on; }
   bool getFused() const { return fused_; }

   void solve( const OperatorType& A, const FunctionType& x, const FunctionType& b, uint_t level ) override
   {
      checkLevel( level );
      const std::vector< double >& c = coefficients_[level - minLevel_];
      if ( c.empty() )
         throw std::runtime_error( "ChebyshevSmoother::solve: coefficients have not been set up on this level" );
      prepareTemporaries( x, level );
      if constexpr ( HasChebyshevSteps< OperatorType, FunctionType >::value )
      {
         if ( fused_ && A.chebyshevFusable( level ) )
         {
            const FunctionType *tIn = &tmp1_, *tOut = &tmp2_;
            A.chebyshevStart( *tIn, b, x, c[0], level, flag_ );
            for ( size_t k = 1; k < c.size(); ++k )
            {
               A.chebyshevStep( *tOut, x, *tIn, c[k - 1], c[k], k == 1, level, flag_ );
               std::swap( tIn, tOut );
            }
            if ( c.size() == 1 )
               A.chebyshevFinish( x, *tIn, c[0], level, flag_ );
            return;
         }
      }
      const auto& invDiag = *A.getInverseDiagonalValues();
      A.apply( x, tmp2_, level, flag_ );
      tmp2_.assign( { 1.0, -1.0 }, { b, tmp2_ }, level, flag_ );
      tmp1_.multElementwise( { invDiag, tmp2_ }, level, flag_ );
      x.assign( { 1.0, c[0] }, { x, tmp1_ }, level, flag_ );
      for ( size_t k = 1; k < c.size(); ++k )
      {
         A.apply( tmp1_, tmp2_, level, flag_ );
         tmp1_.multElementwise( { invDiag, tmp2_ }, level, flag_ );
         x.assign( { 1.0, c[k] }, { x, tmp1_ }, level, flag_ );
      }
   }

 private:
   void checkLevel( uint_t level ) const
   {
      if ( level < minLevel_ || level > maxLevel_ )
         throw std::runtime_error( "ChebyshevSmoother: level needs to be within minLevel and maxLevel" );
   }
   // copyBCs( x, tmp ) of the reference, and zero on the points the flag does not select
   void prepareTemporaries( const FunctionType& x, uint_t level )
   {
      tmp1_.copyBoundaryConditionFromFunction( x );
      tmp2_.copyBoundaryConditionFromFunction( x );
      const SelectionType             selected = x.effectiveFlag( flag_ );
      std::optional< SelectionType >& last     = lastSelection_[level - minLevel_];
      if ( last && *last != selected )
      {
         tmp1_.setToZero( level );
         tmp2_.setToZero( level );
      }
      last = selected;
   }

   DoFType                                   flag_;
   uint_t                                    minLevel_, maxLevel_;
   FunctionType                              tmp1_, tmp2_;
   std::vector< std::vector< double > >      coefficients_;
   // a Selection, or one per component of a vector function
   using SelectionType = decltype( std::declval< const FunctionType& >().effectiveFlag( std::declval< const Selection& >() ) );
   std::vector< std::optional< SelectionType > > lastSelection_; // per level: what the temporaries were last written under
   bool                                      fused_ = true;
};

} // namespace hyteg
