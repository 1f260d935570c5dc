// taylorhood.hpp -- part of the C++ host layer above the C-ABI (see hyteg_host.hpp for the data model).
// P2-P1 Taylor-Hood Stokes composition (BASELINE config 5's "P2-P1 Stokes block operator"): the two mixed forms and the
// P2 -> P1 / P1 -> P2 operators are written here; everything composed of them is the templates of stokes.hpp instantiated with a
// P2 velocity (the aliases at the end of this file).
//   P2ToP1 / P1ToP2 mixed operators   src/mixed_operator/P2ToP1ConstantOperator.hpp:47-101, P1ToP2ConstantOperator.hpp
//   P2P1TaylorHoodFunction            src/hyteg/composites/P2P1TaylorHoodFunction.hpp
//   P2P1TaylorHoodStokesOperator      src/mixed_operator/P2P1TaylorHoodStokesOperator.hpp:34-110
//   transfer                          src/hyteg/gridtransferoperators/P2P1StokesToP2P1Stokes{Restriction,Prolongation}.hpp
// No new device code: a P2 -> P1 block is the P2 apply kernel asked for its vertex-DoF rows only, with an element matrix whose
// edge rows are zero; a P1 -> P2 block is the same kernel with zero edge columns and a zero edge-DoF source array.
#pragma once

#include "minres.hpp"
#include "p2operator.hpp"
#include "p2gridtransfer.hpp"
#include "stokes.hpp"

namespace hyteg {

namespace forms {
// int_T lambda_i d_k phi_j (i: P1 shape function, j: P2 shape function in FEniCS ordering: vertices 0-3, edges (2,3) (1,3) (1,2) (0,3)
// (0,2) (0,1)) in closed form: phi_a = lambda_a ( 2 lambda_a - 1 ), phi_ab = 4 lambda_a lambda_b,
// int lambda_i = V / 4, int lambda_i lambda_p = V ( 1 + delta_ip ) / 20.
inline void p2GradientAgainstP1( const std::array< Point3D, 4 >& c, int k, double B[4][10] )
{
   double J[3][3];
   for ( int r = 0; r < 3; ++r )
      for ( int q = 0; q < 3; ++q )
         J[r][q] = c[q + 1][r] - c[0][r];
   const double det = det3( J );
   double       Ji[3][3];
   Ji[0][0] = ( J[1][1] * J[2][2] - J[1][2] * J[2][1] ) / det;
   Ji[0][1] = ( J[0][2] * J[2][1] - J[0][1] * J[2][2] ) / det;
   Ji[0][2] = ( J[0][1] * J[1][2] - J[0][2] * J[1][1] ) / det;
   Ji[1][0] = ( J[1][2] * J[2][0] - J[1][0] * J[2][2] ) / det;
   Ji[1][1] = ( J[0][0] * J[2][2] - J[0][2] * J[2][0] ) / det;
   Ji[1][2] = ( J[0][2] * J[1][0] - J[0][0] * J[1][2] ) / det;
   Ji[2][0] = ( J[1][0] * J[2][1] - J[1][1] * J[2][0] ) / det;
   Ji[2][1] = ( J[0][1] * J[2][0] - J[0][0] * J[2][1] ) / det;
   Ji[2][2] = ( J[0][0] * J[1][1] - J[0][1] * J[1][0] ) / det;
   double g[4]; // d_k lambda_a
   g[1] = Ji[0][k], g[2] = Ji[1][k], g[3] = Ji[2][k];
   g[0] = -( g[1] + g[2] + g[3] );
   const double     V           = std::fabs( det ) / 6.0;
   static const int pairs[6][2] = { { 2, 3 }, { 1, 3 }, { 1, 2 }, { 0, 3 }, { 0, 2 }, { 0, 1 } };
   for ( int i = 0; i < 4; ++i )
   {
      for ( int a = 0; a < 4; ++a ) // grad phi_a = ( 4 lambda_a - 1 ) grad lambda_a
         B[i][a] = g[a] * V * ( i == a ? 3.0 / 20.0 : -1.0 / 20.0 );
      for ( int e = 0; e < 6; ++e ) // grad phi_ab = 4 ( lambda_b grad lambda_a + lambda_a grad lambda_b )
      {
         const int a = pairs[e][0], b = pairs[e][1];
         B[i][4 + e] = 4.0 * V / 20.0 * ( g[a] * ( i == b ? 2.0 : 1.0 ) + g[b] * ( i == a ? 2.0 : 1.0 ) );
      }
   }
}
// p2_to_p1_tet_div_tet_cell_integral_K_otherwise ( - int q d_K u ) as a 10 x 10 matrix whose edge ROWS are zero
template < int K >
struct P2ToP1DivForm
{
   static void integrateAll( const std::array< Point3D, 4 >& c, double elMat[100] )
   {
      double B[4][10];
      p2GradientAgainstP1( c, K, B );
      for ( int k = 0; k < 100; ++k )
         elMat[k] = 0.0;
      for ( int i = 0; i < 4; ++i )
         for ( int j = 0; j < 10; ++j )
            elMat[10 * i + j] = -B[i][j];
   }
};
// p1_to_p2_tet_divt_tet_cell_integral_K_otherwise ( - int p d_K v ) as a 10 x 10 matrix whose edge COLUMNS are zero
template < int K >
struct P1ToP2DivTForm
{
   static void integrateAll( const std::array< Point3D, 4 >& c, double elMat[100] )
   {
      double B[4][10];
      p2GradientAgainstP1( c, K, B );
      for ( int k = 0; k < 100; ++k )
         elMat[k] = 0.0;
      for ( int j = 0; j < 10; ++j )
         for ( int i = 0; i < 4; ++i )
            elMat[10 * j + i] = -B[i][j];
   }
};
} // namespace forms

// P2ToP1ConstantOperator< Form > (P2ToP1ConstantOperator.hpp:47): dst( P1 ) = / += A src( P2 )
template < class Form >
class P2ToP1Operator : public P2ElementwiseOperator< Form >
{
   using Base = P2ElementwiseOperator< Form >;

 public:
   using srcType = P2Function< double >;
   using dstType = P1Function< double >;
   P2ToP1Operator( const std::shared_ptr< PrimitiveStorage >& storage, uint_t minLevel, uint_t maxLevel )
   : Base( storage, minLevel, maxLevel )
   , tmp_( "p2_to_p1_tmp", storage, minLevel, maxLevel )
   , tmpP1_( "p2_to_p1_tmp_p1", storage, minLevel, maxLevel )
   {}
   void apply( const srcType& src, const dstType& dst, uint_t level, const Selection& flagIn, UpdateType updateType = Replace ) const
   {
      const Selection flag = dst.effectiveFlag( flagIn ); // the destination's boundary condition decides; the temporary follows it
      std::vector< double* >       dv, de;
      std::vector< const double* > sv, se;
      for ( uint_t c = 0; c < this->storage_->getNumberOfLocalCells(); ++c )
      {
         dv.push_back( tmpP1_.getCellPointer( c, level ) ), de.push_back( tmp_.getEdgeCellPointer( c, level ) );
         sv.push_back( src.getVertexDoFFunction().getCellPointer( c, level ) ), se.push_back( src.getEdgeCellPointer( c, level ) );
      }
      this->launchPointers( this->elementMatrices_.at( level ), 1.0, sv, se, dv, de, level, this->storage_->masksFor( flag ), HYTEG_HIP_REPLACE, 1u );
      if ( this->storage_->getCells().size() > 1 )
         tmpP1_.sumSharedCopies( level, flag );
      if ( updateType == Replace )
         dst.assign( { 1.0 }, { tmpP1_ }, level, flag );
      else
         dst.add( { 1.0 }, { tmpP1_ }, level, flag );
   }

 private:
   P2Function< double >         tmp_; // its edge array is the (never written) edge destination the kernel's signature asks for
   mutable P1Function< double > tmpP1_;
};

// P1ToP2ConstantOperator< Form > (P1ToP2ConstantOperator.hpp): dst( P2 ) = / += A src( P1 )
template < class Form >
class P1ToP2Operator : public P2ElementwiseOperator< Form >
{
   using Base = P2ElementwiseOperator< Form >;

 public:
   using srcType = P1Function< double >;
   using dstType = P2Function< double >;
   P1ToP2Operator( const std::shared_ptr< PrimitiveStorage >& storage, uint_t minLevel, uint_t maxLevel )
   : Base( storage, minLevel, maxLevel )
   , tmp_( "p1_to_p2_tmp", storage, minLevel, maxLevel )
   , zero_( "p1_to_p2_zero", storage, minLevel, maxLevel )
   {}
   void apply( const srcType& src, const dstType& dst, uint_t level, const Selection& flagIn, UpdateType updateType = Replace ) const
   {
      const Selection flag = dst.effectiveFlag( flagIn ); // the destination's boundary condition decides; the temporary follows it
      std::vector< double* >       dv, de;
      std::vector< const double* > sv, se;
      for ( uint_t c = 0; c < this->storage_->getNumberOfLocalCells(); ++c )
      {
         dv.push_back( tmp_.getVertexDoFFunction().getCellPointer( c, level ) ), de.push_back( tmp_.getEdgeCellPointer( c, level ) );
         sv.push_back( src.getCellPointer( c, level ) ), se.push_back( zero_.getEdgeCellPointer( c, level ) );
      }
      this->launchPointers( this->elementMatrices_.at( level ), 1.0, sv, se, dv, de, level, this->storage_->masksFor( flag ), HYTEG_HIP_REPLACE, 0xFFu );
      if ( this->storage_->getCells().size() > 1 )
      {
         tmp_.getVertexDoFFunction().sumSharedCopies( level, flag );
         tmp_.sumSharedEdgeCopies( level, flag );
      }
      if ( updateType == Replace )
         dst.assign( { 1.0 }, { tmp_ }, level, flag );
      else
         dst.add( { 1.0 }, { tmp_ }, level, flag );
   }

 private:
   P2Function< double > tmp_;
   P2Function< double > zero_; // zero edge-DoF source (the element matrix has zero edge columns; the kernel still reads the array)
};

// The composition of stokes.hpp with a P2 velocity:
// P2VectorFunction (src/hyteg/p2functionspace/P2VectorFunction.hpp), three components
template < typename ValueType >
using P2VectorFunction = VectorFunction< P2Function< ValueType > >;
// P2P1TaylorHoodFunction (composites/P2P1TaylorHoodFunction.hpp): P2 velocity with the storage's boundary types, P1 pressure with
// createAllInnerBC
template < typename ValueType >
using P2P1TaylorHoodFunction = StokesFunction< P2Function< ValueType > >;
// the three div / divT blocks as one operator (VectorToScalarOperator / ScalarToVectorOperator, src/mixed_operator/)
using P2ToP1DivOperator =
    VectorToScalarOperator< P2ToP1Operator< forms::P2ToP1DivForm< 0 > >, P2ToP1Operator< forms::P2ToP1DivForm< 1 > >, P2ToP1Operator< forms::P2ToP1DivForm< 2 > > >;
using P1ToP2DivTOperator =
    ScalarToVectorOperator< P1ToP2Operator< forms::P1ToP2DivTForm< 0 > >, P1ToP2Operator< forms::P1ToP2DivTForm< 1 > >, P1ToP2Operator< forms::P1ToP2DivTForm< 2 > > >;
// P2ConstantVectorLaplaceOperator (VectorLaplaceOperator.hpp): the scalar operator on every component
using P2ConstantVectorLaplaceOperator = VectorLaplaceOperator< P2ConstantLaplaceOperator >;
// P2P1TaylorHoodStokesOperator.hpp:34-110 (apply :55-64; no PSPG block in the apply: the PSPG members serve the Uzawa smoother as
// Schur-complement approximation)
using P2P1TaylorHoodStokesOperator = StokesOperator< P2ConstantLaplaceOperator, P2ToP1DivOperator, P1ToP2DivTOperator, false >;
// P2P1StokesToP2P1StokesRestriction.hpp / ...Prolongation.hpp: quadratic transfer on the velocity, linear on the pressure
using P2P1StokesToP2P1StokesRestriction  = StokesRestriction< P2toP2QuadraticRestriction >;
using P2P1StokesToP2P1StokesProlongation = StokesProlongation< P2toP2QuadraticProlongation >;

// P1toP2Conversion / P2toP1Conversion of vector functions (P1toP2Conversion.cpp:141-149, P2toP1Conversion.cpp:142-150): component by component
inline void P1toP2Conversion( const P1VectorFunction< double >& src, const P2VectorFunction< double >& dst, const uint_t& P2Level, const Selection& flag = All )
{
   for ( uint_t k = 0; k < src.getDimension(); ++k )
      P1toP2Conversion( src[k], dst[k], P2Level, flag );
}
inline void P2toP1Conversion( const P2VectorFunction< double >& src, const P1VectorFunction< double >& dst, const uint_t& P1Level, const Selection& flag = All )
{
   for ( uint_t k = 0; k < src.getDimension(); ++k )
      P2toP1Conversion( src[k], dst[k], P1Level, flag );
}

} // namespace hyteg
