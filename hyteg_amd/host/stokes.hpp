// stokes.hpp -- part of the C++ host layer above the C-ABI (see hyteg_host.hpp for the data model).
// The Stokes composition layer, written once for both discretisations: the composite functions, the block operators, the
// Stokes operator, its Uzawa smoother and grid transfer are templates over the velocity's scalar function / operator /
// transfer; the pressure is always P1.  This file instantiates them for the stabilised P1-P1 operator (every block a
// P1ConstantOperator< Form > of p1operator.hpp: the same 15-point stencil kernels as for the Laplace operator, with other
// weights); taylorhood.hpp instantiates them for P2-P1 Taylor-Hood.
// src/mixed_operator/P1P1StokesOperator.hpp, VectorLaplaceOperator.hpp, VectorToScalarOperator.hpp,
// ScalarToVectorOperator.hpp, src/hyteg/composites/P1StokesFunction.hpp, src/hyteg/solvers/UzawaSmoother.hpp,
// src/hyteg/solvers/preconditioners/stokes/StokesVelocityBlockBlockDiagonalPreconditioner.hpp,
// src/hyteg/gridtransferoperators/P1P1StokesToP1P1Stokes{Restriction,Prolongation}.hpp.
#pragma once

#include "minres.hpp"
#include "solvers.hpp"

namespace hyteg {

// P1ConstantOperator.hpp:178-210
using P1DivxOperator  = P1ConstantOperator< forms::P1DivForm< 0 > >;
using P1DivyOperator  = P1ConstantOperator< forms::P1DivForm< 1 > >;
using P1DivzOperator  = P1ConstantOperator< forms::P1DivForm< 2 > >;
using P1DivTxOperator = P1ConstantOperator< forms::P1DivTForm< 0 > >;
using P1DivTyOperator = P1ConstantOperator< forms::P1DivTForm< 1 > >;
using P1DivTzOperator = P1ConstantOperator< forms::P1DivTForm< 2 > >;
using P1PSPGOperator  = P1ConstantOperator< forms::P1PSPGForm >;

// =====================================================================================================
// Composite functions
// =====================================================================================================
// P1VectorFunction (src/hyteg/p1functionspace/P1VectorFunction.hpp) / P2VectorFunction
// (src/hyteg/p2functionspace/P2VectorFunction.hpp): three components in 3D
template < class ScalarFunction >
class VectorFunction
{
 public:
   using ValueType = typename ScalarFunction::valueType;
   using Refs      = std::vector< std::reference_wrapper< const VectorFunction > >;
   VectorFunction( const std::string& name, const std::shared_ptr< PrimitiveStorage >& storage, uint_t minLevel, uint_t maxLevel )
   {
      static const char* suffix[3] = { "_u", "_v", "_w" }; // they name timing-tree entries
      for ( int k = 0; k < 3; ++k )
         comp_.push_back( std::make_shared< ScalarFunction >( name + suffix[k], storage, minLevel, maxLevel ) );
   }
   // a view of three existing scalar functions as the components of one vector function (shared ownership)
   explicit VectorFunction( const std::vector< std::shared_ptr< ScalarFunction > >& components )
   : comp_( components )
   {
      if ( comp_.size() != 3 || !comp_[0] || !comp_[1] || !comp_[2] )
         throw std::runtime_error( "VectorFunction: three components" );
   }
   uint_t                getDimension() const { return 3; }
   const ScalarFunction& operator[]( uint_t k ) const { return *comp_.at( k ); }

   // Function::setBoundaryCondition: one condition for all components, or ( bc, k ) for component k alone
   void setBoundaryCondition( const BoundaryCondition& bc )
   {
      for ( auto& c : comp_ )
         c->setBoundaryCondition( bc );
   }
   void setBoundaryCondition( const BoundaryCondition& bc, uint_t k ) { comp_.at( k )->setBoundaryCondition( bc ); }
   // component by component (copyBCs)
   void copyBoundaryConditionFromFunction( const VectorFunction& other )
   {
      for ( uint_t k = 0; k < 3; ++k )
         comp_[k]->copyBoundaryConditionFromFunction( other[k] );
   }

   void interpolate( ValueType constant, uint_t level, DoFType flag = All ) const
   {
      for ( auto& c : comp_ )
         c->interpolate( constant, level, flag );
   }
   void interpolate( const std::vector< std::function< ValueType( const Point3D& ) > >& expr, uint_t level, DoFType flag = All ) const
   {
      for ( uint_t k = 0; k < 3; ++k )
         comp_[k]->interpolate( expr.at( k ), level, flag );
   }
   void assign( const std::vector< ValueType >& scalars, const Refs& functions, uint_t level, DoFType flag = All ) const
   {
      for ( uint_t k = 0; k < 3; ++k )
         comp_[k]->assign( scalars, componentRefs( functions, k ), level, flag );
   }
   void add( const std::vector< ValueType >& scalars, const Refs& functions, uint_t level, DoFType flag = All ) const
   {
      for ( uint_t k = 0; k < 3; ++k )
         comp_[k]->add( scalars, componentRefs( functions, k ), level, flag );
   }
   ValueType dotGlobal( const VectorFunction& rhs, uint_t level, DoFType flag = All ) const
   {
      ValueType s = 0;
      for ( uint_t k = 0; k < 3; ++k )
         s += comp_[k]->dotGlobal( rhs[k], level, flag );
      return s;
   }
   // what the solver templates (solvers.hpp, chebyshev.hpp) ask of their FunctionType beyond the above, component by component
   void multElementwise( const Refs& functions, uint_t level, const Selection& flag = All ) const
   {
      for ( uint_t k = 0; k < 3; ++k )
         comp_[k]->multElementwise( componentRefs( functions, k ), level, flag );
   }
   void setToZero( uint_t level ) const
   {
      for ( auto& c : comp_ )
         c->setToZero( level );
   }
   // the identity of the composite is that of its first component (as a Stokes function's is its pressure's)
   uint64_t uid() const { return comp_[0]->uid(); }
   // one selection per component: each under its own boundary condition
   std::array< Selection, 3 > effectiveFlag( const Selection& s ) const
   {
      return { comp_[0]->effectiveFlag( s ), comp_[1]->effectiveFlag( s ), comp_[2]->effectiveFlag( s ) };
   }

 private:
   static std::vector< std::reference_wrapper< const ScalarFunction > > componentRefs( const Refs& functions, uint_t k )
   {
      std::vector< std::reference_wrapper< const ScalarFunction > > r;
      for ( const auto& f : functions )
         r.push_back( std::cref( f.get()[k] ) );
      return r;
   }
   std::vector< std::shared_ptr< ScalarFunction > > comp_;
};
template < typename ValueType >
using P1VectorFunction = VectorFunction< P1Function< ValueType > >;

// P1StokesFunction (composites/P1StokesFunction.hpp) / P2P1TaylorHoodFunction (composites/P2P1TaylorHoodFunction.hpp):
// velocity with the storage's default boundary condition (create0123BC) unless setVelocityBoundaryCondition gives it another,
// P1 pressure with createAllInnerBC
template < class VelocityScalarFunction >
class StokesFunction
{
 public:
   using valueType = typename VelocityScalarFunction::valueType;
   using ValueType = valueType;
   using Refs      = std::vector< std::reference_wrapper< const StokesFunction > >;
   StokesFunction( const std::string& name, const std::shared_ptr< PrimitiveStorage >& storage, uint_t minLevel, uint_t maxLevel )
   : uvw_( name + "_uvw", storage, minLevel, maxLevel )
   , p_( name + "_p", storage, minLevel, maxLevel )
   {
      p_.setBoundaryConditionAllInner();
   }
   const VectorFunction< VelocityScalarFunction >& uvw() const { return uvw_; }
   const P1Function< ValueType >&                  p() const { return p_; }
   uint64_t                                        uid() const { return p_.uid(); }
   // the boundary condition of the velocity: all components, or component k alone.  The pressure stays all-inner
   // (composites/P1StokesFunction.hpp:41-42).  To be set before a multigrid solver records launch graphs with this function: the
   // composite's identity is that of its pressure
   void setVelocityBoundaryCondition( const BoundaryCondition& bc ) { uvw_.setBoundaryCondition( bc ); }
   void setVelocityBoundaryCondition( const BoundaryCondition& bc, uint_t k ) { uvw_.setBoundaryCondition( bc, k ); }
   void copyBoundaryConditionFromFunction( const StokesFunction& other )
   {
      uvw_.copyBoundaryConditionFromFunction( other.uvw() );
      p_.copyBoundaryConditionFromFunction( other.p() );
   }

   void interpolate( ValueType constant, uint_t level, DoFType flag = All ) const
   {
      uvw_.interpolate( constant, level, flag );
      p_.interpolate( constant, level, flag );
   }
   void assign( const std::vector< ValueType >& scalars, const Refs& functions, uint_t level, DoFType flag = All ) const
   {
      const auto parts = split( functions );
      uvw_.assign( scalars, parts.first, level, flag );
      p_.assign( scalars, parts.second, level, flag );
   }
   void add( const std::vector< ValueType >& scalars, const Refs& functions, uint_t level, DoFType flag = All ) const
   {
      const auto parts = split( functions );
      uvw_.add( scalars, parts.first, level, flag );
      p_.add( scalars, parts.second, level, flag );
   }
   ValueType dotGlobal( const StokesFunction& rhs, uint_t level, DoFType flag = All ) const
   {
      return uvw_.dotGlobal( rhs.uvw(), level, flag ) + p_.dotGlobal( rhs.p(), level, flag );
   }

 private:
   using PressureRefs = std::vector< std::reference_wrapper< const P1Function< ValueType > > >;
   // the velocities and the pressures of a list of functions
   static std::pair< typename VectorFunction< VelocityScalarFunction >::Refs, PressureRefs > split( const Refs& functions )
   {
      std::pair< typename VectorFunction< VelocityScalarFunction >::Refs, PressureRefs > parts;
      for ( const auto& f : functions )
      {
         parts.first.push_back( std::cref( f.get().uvw() ) );
         parts.second.push_back( std::cref( f.get().p() ) );
      }
      return parts;
   }
   VectorFunction< VelocityScalarFunction > uvw_;
   P1Function< ValueType >                  p_;
};
template < typename ValueType >
using P1StokesFunction = StokesFunction< P1Function< ValueType > >;

// vertexdof::projectMean (VertexDoFFunction.hpp:586-592): subtract the mean over ALL DoFs (every shared DoF counted once)
inline void projectMean( const P1Function< double >& pressure, uint_t level )
{
   auto                 storage = pressure.getStorage();
   P1Function< double > one( "projectMean_one", storage, level, level );
   one.interpolate( 1.0, level, All );
   const double count = one.dotGlobal( one, level, All );
   const double sum   = pressure.dotGlobal( one, level, All );
   pressure.add( { -sum / count }, { one }, level, All );
}

// =====================================================================================================
// Block operators
// =====================================================================================================
// VectorLaplaceOperator.hpp:122  P1ConstantVectorLaplaceOperator / P2ConstantVectorLaplaceOperator: block diagonal of one
// scalar Laplace operator
template < class ScalarOperator >
class VectorLaplaceOperator
{
 public:
   using srcType = VectorFunction< typename ScalarOperator::srcType >;
   using dstType = srcType;
   VectorLaplaceOperator( const std::shared_ptr< PrimitiveStorage >& storage, uint_t minLevel, uint_t maxLevel )
   : lapl_( storage, minLevel, maxLevel )
   {
      lapl_.computeInverseDiagonalOperatorValues(); // Jacobi-type velocity smoothers ask the scalar operator for it
   }
   void apply( const srcType& src, const dstType& dst, uint_t level, DoFType flag, UpdateType updateType = Replace ) const
   {
      for ( uint_t k = 0; k < 3; ++k )
         lapl_.apply( src[k], dst[k], level, flag, updateType );
   }
   const ScalarOperator& getSubOperator( uint_t, uint_t ) const { return lapl_; }

 private:
   ScalarOperator lapl_;
};
using P1ConstantVectorLaplaceOperator = VectorLaplaceOperator< P1ConstantLaplaceOperator >;

// VectorToScalarOperator.hpp: ( X, Y, Z ): first component with the caller's update type, the others added (:63-71)
template < class X, class Y, class Z >
class VectorToScalarOperator
{
 public:
   VectorToScalarOperator( const std::shared_ptr< PrimitiveStorage >& storage, uint_t minLevel, uint_t maxLevel )
   : x_( storage, minLevel, maxLevel )
   , y_( storage, minLevel, maxLevel )
   , z_( storage, minLevel, maxLevel )
   {}
   void apply( const VectorFunction< typename X::srcType >& src, const typename X::dstType& dst, uint_t level, DoFType flag,
               UpdateType updateType = Replace ) const
   {
      x_.apply( src[0], dst, level, flag, updateType );
      y_.apply( src[1], dst, level, flag, Add );
      z_.apply( src[2], dst, level, flag, Add );
   }

 private:
   X x_;
   Y y_;
   Z z_;
};
// ScalarToVectorOperator.hpp: ( X, Y, Z )^T
template < class X, class Y, class Z >
class ScalarToVectorOperator
{
 public:
   ScalarToVectorOperator( const std::shared_ptr< PrimitiveStorage >& storage, uint_t minLevel, uint_t maxLevel )
   : x_( storage, minLevel, maxLevel )
   , y_( storage, minLevel, maxLevel )
   , z_( storage, minLevel, maxLevel )
   {}
   void apply( const typename X::srcType& src, const VectorFunction< typename X::dstType >& dst, uint_t level, DoFType flag,
               UpdateType updateType = Replace ) const
   {
      x_.apply( src, dst[0], level, flag, updateType );
      y_.apply( src, dst[1], level, flag, updateType );
      z_.apply( src, dst[2], level, flag, updateType );
   }

 private:
   X x_;
   Y y_;
   Z z_;
};
using P1ConstantDivOperator  = VectorToScalarOperator< P1DivxOperator, P1DivyOperator, P1DivzOperator >;
using P1ConstantDivTOperator = ScalarToVectorOperator< P1DivTxOperator, P1DivTyOperator, P1DivTzOperator >;

// P1PSPGInvDiagOperator (P1ConstantOperator.hpp:206-210: Diagonal, InvertDiagonal): the stencil keeps only the centre
// weight, inverted (P1Operator.hpp:2149-2158; on shared points the inverse of the SUM over the neighbour cells, :2110-2117)
// = pointwise multiplication with the inverse diagonal of the PSPG operator
class P1PSPGInvDiagOperator
{
 public:
   P1PSPGInvDiagOperator( const std::shared_ptr< PrimitiveStorage >& storage, uint_t minLevel, uint_t maxLevel )
   : pspg_( storage, minLevel, maxLevel )
   , tmp_( "pspg_inv_diag_tmp", storage, minLevel, maxLevel )
   {
      pspg_.computeInverseDiagonalOperatorValues();
      tmp_.setBoundaryConditionAllInner();
   }
   void apply( const P1Function< double >& src, const P1Function< double >& dst, uint_t level, DoFType flag, UpdateType updateType = Replace ) const
   {
      applyPointwiseScaling( *pspg_.getInverseDiagonalValues(), tmp_, src, dst, level, flag, updateType );
   }

 private:
   P1PSPGOperator       pspg_;
   P1Function< double > tmp_;
};

// P1P1StokesOperator.hpp:32-99 / P2P1TaylorHoodStokesOperator.hpp:34-110: the velocity's scalar Laplace operator on every
// component, the div and divT blocks, and the PSPG block -- applied by a stabilised operator only; its members serve the Uzawa
// smoother of both as Schur-complement approximation
template < class VelocityOperator, class DivOperator, class DivTOperator, bool HasPspgBlock >
class StokesOperator
{
 public:
   using srcType            = StokesFunction< typename VelocityOperator::srcType >;
   using dstType            = srcType;
   using VelocityOperator_T = VelocityOperator;
   // has_pspg_block< P1P1StokesOperator > (P1P1StokesOperator.hpp:95); no specialisation for the Taylor-Hood operator
   // (StokesOperatorTraits.hpp:25-29)
   static constexpr bool hasPspgBlock = HasPspgBlock;

   StokesOperator( const std::shared_ptr< PrimitiveStorage >& storage, uint_t minLevel, uint_t maxLevel )
   : lapl( storage, minLevel, maxLevel )
   , div( storage, minLevel, maxLevel )
   , divT( storage, minLevel, maxLevel )
   , pspg( storage, minLevel, maxLevel )
   , pspg_inv_diag_( storage, minLevel, maxLevel )
   , storage_( storage )
   {}

   // P1P1StokesOperator.hpp:51-64, P2P1TaylorHoodStokesOperator.hpp:55-64
   void apply( const srcType& src, const dstType& dst, uint_t level, DoFType flag, UpdateType = Replace ) const
   {
      if ( &src == &dst )
         throw std::runtime_error( "StokesOperator::apply: src and dst must differ" );
      lapl.apply( src.uvw(), dst.uvw(), level, flag, Replace );
      divT.apply( src.p(), dst.uvw(), level, flag, Add );
      div.apply( src.uvw(), dst.p(), level, flag, Replace );
      if constexpr ( hasPspgBlock )
         pspg.apply( src.p(), dst.p(), level, flag, Add );
   }
   const VelocityOperator&             getA() const { return lapl.getSubOperator( 0, 0 ); }
   std::shared_ptr< PrimitiveStorage > getStorage() const { return storage_; }
   uint64_t                            uid() const { return uid_; }

   VectorLaplaceOperator< VelocityOperator > lapl;
   DivOperator                               div;
   DivTOperator                              divT;
   P1PSPGOperator                            pspg;
   P1PSPGInvDiagOperator                     pspg_inv_diag_;

 private:
   std::shared_ptr< PrimitiveStorage > storage_;
   uint64_t                            uid_ = nextUid();
};
using P1P1StokesOperator = StokesOperator< P1ConstantLaplaceOperator, P1ConstantDivOperator, P1ConstantDivTOperator, true >;

// =====================================================================================================
// Smoothers and grid transfer
// =====================================================================================================
// StokesVelocityBlockBlockDiagonalPreconditioner.hpp:34-56: the scalar smoother on every velocity component
template < class OperatorType >
class StokesVelocityBlockBlockDiagonalPreconditioner : public Solver< OperatorType >
{
 public:
   using FunctionType = typename OperatorType::srcType;
   StokesVelocityBlockBlockDiagonalPreconditioner( const std::shared_ptr< PrimitiveStorage >&,
                                                   std::shared_ptr< Solver< typename OperatorType::VelocityOperator_T > > scalar )
   : scalar_( std::move( scalar ) )
   {}
   void solve( const OperatorType& A, const FunctionType& x, const FunctionType& b, uint_t level ) override
   {
      // the components are independent: one solveMany instead of a loop, so that a smoother can sweep them with shared launches
      // (the P1 SOR smoothers do; every other smoother's solveMany is the loop of solve() calls)
      std::vector< std::reference_wrapper< const typename OperatorType::VelocityOperator_T::srcType > > xs, bs;
      for ( uint_t k = 0; k < x.uvw().getDimension(); ++k )
      {
         xs.push_back( std::cref( x.uvw()[k] ) );
         bs.push_back( std::cref( b.uvw()[k] ) );
      }
      scalar_->solveMany( A.getA(), xs, bs, level );
   }

 private:
   std::shared_ptr< Solver< typename OperatorType::VelocityOperator_T > > scalar_;
};

// UzawaSmoother.hpp:99-330, block-Laplace variant with PSPG stabilisation (:262-288):
//   r.uvw = b.uvw - divT x.p;   numGSIterationsVelocity x velocitySmoother( A, x, r );
//   r.p   = relax * ( b.p - ( pspg x.p + div x.uvw ) );   x.p += pspg_inv_diag r.p
template < class OperatorType >
class UzawaSmoother : public Solver< OperatorType >
{
 public:
   using FunctionType = typename OperatorType::srcType;
   UzawaSmoother( const std::shared_ptr< PrimitiveStorage >& storage,
                  std::shared_ptr< Solver< OperatorType > >  velocitySmoother,
                  uint_t                                     minLevel,
                  uint_t                                     maxLevel,
                  double                                     relaxParam,
                  DoFType                                    flag                    = Inner | NeumannBoundary | FreeslipBoundary,
                  uint_t                                     numGSIterationsVelocity = 2 )
   : velocitySmoother_( std::move( velocitySmoother ) )
   , flag_( flag )
   , relaxParam_( relaxParam )
   , numGSIterationsVelocity_( numGSIterationsVelocity )
   , r_( "uzawa_smoother_r", storage, minLevel, maxLevel )
   {}
   void setRelaxationParameter( double omega ) { relaxParam_ = omega; }

   void solve( const OperatorType& A, const FunctionType& x, const FunctionType& b, uint_t level ) override
   {
      r_.copyBoundaryConditionFromFunction( x ); // copyBCs
      A.divT.apply( x.p(), r_.uvw(), level, flag_, Replace );
      r_.uvw().assign( { 1.0, -1.0 }, { b.uvw(), r_.uvw() }, level, flag_ );
      for ( uint_t i = 0; i < numGSIterationsVelocity_; ++i )
         velocitySmoother_->solve( A, x, r_, level );
      // has_pspg_block (composites/StokesOperatorTraits.hpp): with a stabilised operator the pressure residual contains C p
      // (UzawaSmoother.hpp:262-288), without one -- Taylor-Hood -- it is b.p - div u (:390-450); both scale it with the inverse
      // diagonal of the PSPG operator
      if constexpr ( OperatorType::hasPspgBlock )
      {
         A.pspg.apply( x.p(), r_.p(), level, flag_, Replace );
         A.div.apply( x.uvw(), r_.p(), level, flag_, Add );
      }
      else
         A.div.apply( x.uvw(), r_.p(), level, flag_, Replace );
      r_.p().assign( { 1.0, -1.0 }, { b.p(), r_.p() }, level, flag_ );
      r_.p().assign( { relaxParam_ }, { r_.p() }, level, flag_ );
      A.pspg_inv_diag_.apply( r_.p(), x.p(), level, flag_, Add );
   }

 private:
   std::shared_ptr< Solver< OperatorType > > velocitySmoother_;
   DoFType                                   flag_;
   double                                    relaxParam_;
   uint_t                                    numGSIterationsVelocity_;
   FunctionType                              r_;
};

// P1P1StokesToP1P1StokesRestriction.hpp:34-58 / ...Prolongation.hpp, P2P1StokesToP2P1StokesRestriction.hpp / ...Prolongation.hpp:
// the velocity's transfer on every component, the linear P1 transfer on the pressure
template < class VelocityRestriction >
class StokesRestriction
{
 public:
   explicit StokesRestriction( bool projectMeanAfterRestriction = false )
   : projectMean_( projectMeanAfterRestriction )
   {}
   template < class FunctionType >
   void restrict( const FunctionType& f, uint_t sourceLevel, DoFType flag ) const
   {
      for ( uint_t k = 0; k < 3; ++k )
         rv_.restrict( f.uvw()[k], sourceLevel, flag );
      rp_.restrict( f.p(), sourceLevel, flag );
      if ( projectMean_ )
         projectMean( f.p(), sourceLevel - 1 );
   }

 private:
   VelocityRestriction     rv_;
   P1toP1LinearRestriction rp_;
   bool                    projectMean_;
};
template < class VelocityProlongation >
class StokesProlongation
{
 public:
   template < class FunctionType >
   void prolongate( const FunctionType& f, uint_t sourceLevel, DoFType flag ) const
   {
      for ( uint_t k = 0; k < 3; ++k )
         pv_.prolongate( f.uvw()[k], sourceLevel, flag );
      pp_.prolongate( f.p(), sourceLevel, flag );
   }
   template < class FunctionType >
   void prolongateAndAdd( const FunctionType& f, uint_t sourceLevel, DoFType flag ) const
   {
      for ( uint_t k = 0; k < 3; ++k )
         pv_.prolongateAndAdd( f.uvw()[k], sourceLevel, flag );
      pp_.prolongateAndAdd( f.p(), sourceLevel, flag );
   }

 private:
   VelocityProlongation     pv_;
   P1toP1LinearProlongation pp_;
};
// P1VectorFunctionLinearRestriction.hpp / P1VectorFunctionLinearProlongation.hpp: the scalar transfer on every component of a
// vector function (the grid transfer of a multigrid cycle on an operator that couples the components)
template < class ScalarRestriction >
class VectorFunctionRestriction
{
 public:
   template < class FunctionType >
   void restrict( const FunctionType& f, uint_t sourceLevel, DoFType flag ) const
   {
      for ( uint_t k = 0; k < f.getDimension(); ++k )
         r_.restrict( f[k], sourceLevel, flag );
   }

 private:
   ScalarRestriction r_;
};
template < class ScalarProlongation >
class VectorFunctionProlongation
{
 public:
   template < class FunctionType >
   void prolongate( const FunctionType& f, uint_t sourceLevel, DoFType flag ) const
   {
      for ( uint_t k = 0; k < f.getDimension(); ++k )
         p_.prolongate( f[k], sourceLevel, flag );
   }
   template < class FunctionType >
   void prolongateAndAdd( const FunctionType& f, uint_t sourceLevel, DoFType flag ) const
   {
      for ( uint_t k = 0; k < f.getDimension(); ++k )
         p_.prolongateAndAdd( f[k], sourceLevel, flag );
   }

 private:
   ScalarProlongation p_;
};
using P1VectorFunctionLinearRestriction  = VectorFunctionRestriction< P1toP1LinearRestriction >;
using P1VectorFunctionLinearProlongation = VectorFunctionProlongation< P1toP1LinearProlongation >;

using P1P1StokesToP1P1StokesRestriction  = StokesRestriction< P1toP1LinearRestriction >;
using P1P1StokesToP1P1StokesProlongation = StokesProlongation< P1toP1LinearProlongation >;

// Coarse-grid solver of the saddle-point system, standing in for PETScLUSolver< P1P1StokesOperator >
// (src/hyteg/petsc/PETScLUSolver.hpp; the convergence tests use it on level 2): the level's operator is assembled into a
// dense matrix by applying it to unit vectors (setup, once per level: 4 x #points applications of a few hundred points
// each), factorised on the host with partial pivoting, and every solve is a download, two triangular solves and an
// upload.  The pressure is determined up to a constant: the matrix is bordered with the zero-mean constraint.
// Single rank only (a coarse-grid direct solve across ranks would gather the system; not needed by the tests here).
template < class OperatorType >
class DenseCoarseGridSolver : public Solver< OperatorType >
{
 public:
   using FunctionType = typename OperatorType::srcType;
   DenseCoarseGridSolver( const std::shared_ptr< PrimitiveStorage >& storage, uint_t level )
   : storage_( storage )
   , level_( level )
   , e_( "dense_coarse_e", storage, level, level )
   , Ae_( "dense_coarse_Ae", storage, level, level )
   {
      if ( storage->numRanks() != 1 )
         throw std::runtime_error( "DenseCoarseGridSolver: single rank only" );
   }

   void solve( const OperatorType& A, const FunctionType& x, const FunctionType& b, uint_t level ) override
   {
      if ( level != level_ )
         throw std::runtime_error( "DenseCoarseGridSolver: built for another level" );
      // the matrix holds identity rows where x's boundary conditions fix a DoF: factorised for them, and again if they change
      if ( !factorised_ || !sameConditions( x ) )
      {
         e_.copyBoundaryConditionFromFunction( x ); // copyBCs
         Ae_.copyBoundaryConditionFromFunction( x );
         for ( uint_t c = 0; c < 4; ++c )
            conditions_[c] = comp( x, c ).boundaryConditionOrNull();
         factorise( A );
      }
      // right-hand side: b on free DoFs; Dirichlet velocity DoFs keep the value x has there (identity rows)
      std::vector< double > rhs( n_ + 1, 0.0 ), xv = gather( x ), bv = gather( b );
      for ( uint_t i = 0; i < n_; ++i )
         rhs[i] = free_[i] ? bv[i] : xv[i];
      // forward / backward substitution with the stored LU factors
      std::vector< double > y( n_ + 1 );
      for ( uint_t i = 0; i <= n_; ++i )
      {
         double s = rhs[perm_[i]];
         for ( uint_t j = 0; j < i; ++j )
            s -= lu_[i * ( n_ + 1 ) + j] * y[j];
         y[i] = s;
      }
      for ( uint_t ii = n_ + 1; ii-- > 0; )
      {
         double s = y[ii];
         for ( uint_t j = ii + 1; j <= n_; ++j )
            s -= lu_[ii * ( n_ + 1 ) + j] * y[j];
         y[ii] = s / lu_[ii * ( n_ + 1 ) + ii];
      }
      scatter( x, y );
   }

 private:
   // global numbering: component c (0..2 velocity, 3 pressure) x global point; a global point = one representative
   // (local cell, array index) per group of copies, found through the exchange-free property that copies agree
   struct PointRef
   {
      uint_t cell;
      int    index;
   };
   void enumeratePoints()
   {
      const int64_t N = layout::width( (int) level_ ), total = layout::cellSize( (int) level_ );
      const uint_t  nCells = storage_->getNumberOfLocalCells();
      // identify copies by their physical coordinates (exact in binary for the dyadic refinement of one macro-vertex set:
      // use the barycentric integer coordinates with the GLOBAL macro-vertex ids, sorted)
      std::map< std::vector< int64_t >, uint_t > ids;
      pointOf_.assign( nCells, std::vector< int >( (size_t) total, -1 ) );
      for ( uint_t c = 0; c < nCells; ++c )
      {
         const MacroCell& cell = storage_->getLocalCell( c );
         for ( int64_t z = 0; z < N; ++z )
            for ( int64_t y = 0; y < N - z; ++y )
               for ( int64_t x = 0; x < N - z - y; ++x )
               {
                  const int64_t bary[4] = { N - 1 - x - y - z, x, y, z };
                  std::vector< std::pair< int, int64_t > > key;
                  for ( int k = 0; k < 4; ++k )
                     if ( bary[k] != 0 )
                        key.push_back( { cell.v[k], bary[k] } );
                  std::sort( key.begin(), key.end() );
                  std::vector< int64_t > flat;
                  for ( auto& kv : key )
                  {
                     flat.push_back( kv.first );
                     flat.push_back( kv.second );
                  }
                  auto it = ids.find( flat );
                  if ( it == ids.end() )
                  {
                     it = ids.emplace( flat, (uint_t) reps_.size() ).first;
                     reps_.push_back( { c, (int) layout::cellIndex( N, x, y, z ) } );
                  }
                  pointOf_[c][(size_t) layout::cellIndex( N, x, y, z )] = (int) it->second;
               }
      }
      np_ = reps_.size();
      n_  = 4 * np_;
   }
   const P1Function< double >& comp( const FunctionType& f, uint_t c ) const { return c < 3 ? f.uvw()[c] : f.p(); }
   // device-side packing (round 3; the first version moved every cell array through the host by itself: 281,000 synchronous copies
   // at set-up and 288 per coarse-grid solve): index tables built once, one pack launch + one download per gather, one upload +
   // one pack launch per cell array per scatter -- hyteg_hip_gather_entries( out, bases, buf, off, n ): out[k] = bases[buf[k]][off[k]]
   void buildIndexTables() const
   {
      if ( gatherBuf_ )
         return;
      const uint_t      nCells = storage_->getNumberOfLocalCells();
      const int64_t     total  = layout::cellSize( (int) level_ );
      std::vector< int > gb( n_ ), go( n_ );
      for ( uint_t c = 0; c < 4; ++c )
         for ( uint_t g = 0; g < np_; ++g )
         {
            gb[c * np_ + g] = (int) ( c * nCells + reps_[g].cell ); // position of the array in basesOf( f )
            go[c * np_ + g] = reps_[g].index;
         }
      gatherBuf_ = static_cast< const int* >( storage_->uploadBytes( gb.data(), gb.size() * sizeof( int ) ) );
      gatherOff_ = static_cast< const int* >( storage_->uploadBytes( go.data(), go.size() * sizeof( int ) ) );
      // scatter: entry i of the array of (component c, cell) reads V[ c np + pointOf[cell][i] ] -- one table for all components, the
      // component's offset comes through the base pointer V + c np
      std::vector< int > so( nCells * (size_t) total ), zeros( (size_t) total, 0 );
      for ( uint_t cell = 0; cell < nCells; ++cell )
         for ( int64_t i = 0; i < total; ++i )
            so[cell * (size_t) total + (size_t) i] = pointOf_[cell][(size_t) i];
      scatterOff_  = static_cast< const int* >( storage_->uploadBytes( so.data(), so.size() * sizeof( int ) ) );
      scatterZero_ = static_cast< const int* >( storage_->uploadBytes( zeros.data(), zeros.size() * sizeof( int ) ) );
      std::vector< double > none( n_ + 1, 0.0 );
      packed_ = storage_->uploadTable( none );
      std::vector< double* > vb;
      for ( uint_t c = 0; c < 4; ++c )
         vb.push_back( packed_ + c * np_ );
      packedBases_ = storage_->pointerTable( vb );
   }
   double** basesOf( const FunctionType& f ) const
   {
      std::vector< double* > b;
      for ( uint_t c = 0; c < 4; ++c )
         for ( uint_t cell = 0; cell < storage_->getNumberOfLocalCells(); ++cell )
            b.push_back( comp( f, c ).getCellPointer( cell, level_ ) );
      return storage_->pointerTable( b );
   }
   std::vector< double > gather( const FunctionType& f ) const
   {
      buildIndexTables();
      std::vector< double > v( n_ );
      hipCheck( hyteg_hip_gather_entries( packed_, basesOf( f ), gatherBuf_, gatherOff_, (int) n_, storage_->stream() ), "dense coarse solver: gather" );
      hipCheck( hyteg_hip_download( v.data(), packed_, n_ * sizeof( double ), storage_->stream() ), "dense coarse solver: download" );
      hipCheck( hyteg_hip_stream_synchronize( storage_->stream() ), "dense coarse solver: sync" );
      return v;
   }
   // components [cFirst, cLast] of f := v
   void scatter( const FunctionType& f, const std::vector< double >& v, uint_t cFirst = 0, uint_t cLast = 3 ) const
   {
      buildIndexTables();
      const int64_t total = layout::cellSize( (int) level_ );
      hipCheck( hyteg_hip_upload( packed_, v.data(), n_ * sizeof( double ), storage_->stream() ), "dense coarse solver: upload" );
      for ( uint_t c = cFirst; c <= cLast; ++c )
         for ( uint_t cell = 0; cell < storage_->getNumberOfLocalCells(); ++cell )
            hipCheck( hyteg_hip_gather_entries( comp( f, c ).getCellPointer( cell, level_ ), packedBases_ + c, scatterZero_,
                                                scatterOff_ + cell * (size_t) total, (int) total, storage_->stream() ),
                      "dense coarse solver: scatter" );
      hipCheck( hyteg_hip_stream_synchronize( storage_->stream() ), "dense coarse solver: sync" ); // v may go out of scope
   }
   // x's components carry the conditions the factors were computed for (null: the storage's default condition)
   bool sameConditions( const FunctionType& x ) const
   {
      for ( uint_t c = 0; c < 4; ++c )
      {
         const auto bc = comp( x, c ).boundaryConditionOrNull();
         if ( bc != conditions_[c] && !( bc && conditions_[c] && *bc == *conditions_[c] ) )
            return false;
      }
      return true;
   }
   void factorise( const OperatorType& A )
   {
      enumeratePoints();
      const DoFType flag = Inner | NeumannBoundary | FreeslipBoundary;
      // free DoFs: where the operator writes (velocity: not on the Dirichlet boundary; pressure: everywhere)
      {
         e_.interpolate( 0.0, level_, All );
         e_.interpolate( 1.0, level_, flag );
         const auto m = gather( e_ );
         free_.assign( n_, false );
         for ( uint_t i = 0; i < n_; ++i )
            free_[i] = m[i] != 0.0;
      }
      const uint_t          m = n_ + 1;
      std::vector< double > M( m * m, 0.0 );
      std::vector< double > unit( n_, 0.0 );
      scatter( e_, unit );
      for ( uint_t j = 0; j < n_; ++j )
      {
         // only the component that holds DoF j changes (and the previous one when j is a component's first DoF)
         const uint_t c = j / np_;
         if ( j > 0 )
            unit[j - 1] = 0.0;
         unit[j] = 1.0;
         scatter( e_, unit, ( j % np_ == 0 && c > 0 ) ? c - 1 : c, c );
         Ae_.interpolate( 0.0, level_, All );
         A.apply( e_, Ae_, level_, flag );
         const auto col = gather( Ae_ );
         for ( uint_t i = 0; i < n_; ++i )
            M[i * m + j] = free_[i] ? col[i] : ( i == j ? 1.0 : 0.0 );
      }
      // zero-mean pressure: Lagrange multiplier row / column over the pressure DoFs
      for ( uint_t k = 0; k < np_; ++k )
      {
         M[n_ * m + 3 * np_ + k] = 1.0;
         M[( 3 * np_ + k ) * m + n_] = 1.0;
      }
      // LU with partial pivoting; perm_[i] = original row that ended up in row i
      perm_.resize( m );
      for ( uint_t i = 0; i < m; ++i )
         perm_[i] = i;
      for ( uint_t k = 0; k < m; ++k )
      {
         uint_t piv = k;
         for ( uint_t i = k + 1; i < m; ++i )
            if ( std::fabs( M[i * m + k] ) > std::fabs( M[piv * m + k] ) )
               piv = i;
         if ( M[piv * m + k] == 0.0 )
            throw std::runtime_error( "DenseCoarseGridSolver: singular matrix" );
         if ( piv != k )
         {
            for ( uint_t j = 0; j < m; ++j )
               std::swap( M[k * m + j], M[piv * m + j] );
            std::swap( perm_[k], perm_[piv] );
         }
         for ( uint_t i = k + 1; i < m; ++i )
         {
            const double f = M[i * m + k] / M[k * m + k];
            M[i * m + k]   = f;
            if ( f != 0.0 )
               for ( uint_t j = k + 1; j < m; ++j )
                  M[i * m + j] -= f * M[k * m + j];
         }
      }
      lu_.swap( M );
      factorised_ = true;
   }

   std::shared_ptr< PrimitiveStorage > storage_;
   uint_t                              level_;
   FunctionType                        e_, Ae_;
   bool                                factorised_ = false;
   std::shared_ptr< const BoundaryCondition > conditions_[4]; // of the velocity components and the pressure at factorisation
   uint_t                              np_ = 0, n_ = 0;
   std::vector< PointRef >             reps_;
   std::vector< std::vector< int > >   pointOf_;
   std::vector< bool >                 free_;
   std::vector< double >               lu_;
   std::vector< uint_t >               perm_;
   mutable const int *                 gatherBuf_ = nullptr, *gatherOff_ = nullptr, *scatterOff_ = nullptr, *scatterZero_ = nullptr;
   mutable double*                     packed_      = nullptr;
   mutable double**                    packedBases_ = nullptr;
};

} // namespace hyteg
