// p2divkgrad.hpp -- part of the C++ host layer above the C-ABI (see hyteg_host.hpp for the data model).
// P2ElementwiseDivKGrad: the generated variable-coefficient diffusion operator -div( k grad u ) on P2 with a P2 coefficient function,
//    operatorgeneration::P2ElementwiseDivKGrad( storage, minLevel, maxLevel, const P2Function< real_t >& k )
// (module hyteg_operators; call site and known answer: tests/hyteg/convergence/ElementwiseDivKGradCGConvergenceTest.cpp:192-221), and
// forms::P2MassForm, the form of P2ElementwiseMassOperator (P2ElementwiseOperator.hpp) that the known-answer test builds its right-hand
// side with.  The operator has the interface and the schedules of P2ElementwiseOperator (p2operator.hpp): per cell the C-ABI seam
// hyteg_hip_p2_elementwise_divkgrad_apply_cell_kinds, then the additive exchange of the shares of the shared DoFs.  The operator at
// level l reads k at level l: the caller interpolates k on every level it uses, as the reference test does.  No smooth_sor, no constant
// stencils, no fused steps: the solver templates run their composed sequences.
#pragma once

#include "p2operator.hpp"

namespace hyteg {

namespace forms {
// P2 mass element matrix in FEniCS ordering.  Every shape function is a homogeneous quadratic in the barycentric functions,
// phi = sum_cd H_cd l_c l_d ( vertex a: l_a^2 - sum_{c != a} l_a l_c; edge ab: 4 l_a l_b ), and int l^alpha = |e| alpha! / 840 for
// | alpha | = 4, so  M_ij = |e| / 840 sum_cdef H^i_cd H^j_ef alpha!( c, d, e, f ): |e| times universal constants.
struct P2MassForm
{
   static void integrateAll( const std::array< Point3D, 4 >& c, double elMat[100] )
   {
      double g[4][3];
      const double     V           = tetGradients( c, g );
      static const int pairs[6][2] = { { 2, 3 }, { 1, 3 }, { 1, 2 }, { 0, 3 }, { 0, 2 }, { 0, 1 } };
      double           H[10][4][4] = {};
      for ( int a = 0; a < 4; ++a )
         for ( int b = 0; b < 4; ++b )
            H[a][a][b] = H[a][b][a] = a == b ? 1.0 : -0.5;
      for ( int k = 0; k < 6; ++k )
         H[4 + k][pairs[k][0]][pairs[k][1]] = H[4 + k][pairs[k][1]][pairs[k][0]] = 2.0;
      static const double factorial[5] = { 1.0, 1.0, 2.0, 6.0, 24.0 };
      for ( int i = 0; i < 10; ++i )
         for ( int j = 0; j < 10; ++j )
         {
            double s = 0.0;
            for ( int p = 0; p < 4; ++p )
               for ( int q = 0; q < 4; ++q )
                  for ( int e = 0; e < 4; ++e )
                     for ( int f = 0; f < 4; ++f )
                     {
                        int count[4] = { 0, 0, 0, 0 };
                        ++count[p], ++count[q], ++count[e], ++count[f];
                        s += H[i][p][q] * H[j][e][f] * factorial[count[0]] * factorial[count[1]] * factorial[count[2]] * factorial[count[3]];
                     }
            elMat[10 * i + j] = V * s / 840.0;
         }
   }
};
} // namespace forms
using P2ElementwiseMassOperator = P2ElementwiseOperator< forms::P2MassForm >; // P2ElementwiseOperator.hpp

namespace operatorgeneration {

class P2ElementwiseDivKGrad
{
 public:
   using srcType = P2Function< double >;
   using dstType = P2Function< double >;

   P2ElementwiseDivKGrad( const std::shared_ptr< PrimitiveStorage >& storage, uint_t minLevel, uint_t maxLevel, const P2Function< double >& k )
   : storage_( storage )
   , minLevel_( minLevel )
   , maxLevel_( maxLevel )
   , k_( k )
   {
      if ( (int) maxLevel > hyteg_hip_p2_elementwise_divkgrad_max_level() )
         throw std::runtime_error( "P2ElementwiseDivKGrad: levels 0..8" );
      storage->markInUse(); // the mesh boundary flags are fixed from here on
      for ( uint_t l = minLevel; l <= maxLevel; ++l )
         for ( uint_t lc = 0; lc < storage->getNumberOfLocalCells(); ++lc )
         {
            double                   cc[12];
            std::array< double, 60 > g;
            coordsOf( storage->getLocalCell( lc ), cc );
            hipCheck( hyteg_hip_p2_elementwise_divkgrad_geometry( cc, (int) l, g.data() ), "P2ElementwiseDivKGrad: geometry" );
            geometry_[l].push_back( g );
         }
   }
   std::shared_ptr< PrimitiveStorage > getStorage() const { return storage_; }
   uint_t                              getMinLevel() const { return minLevel_; }
   uint_t                              getMaxLevel() const { return maxLevel_; }
   const P2Function< double >&         getCoefficient() const { return k_; }
   uint64_t                            uid() const { return uid_; }

   // Operator::apply = gemv( 1, src, updateType == Replace ? 0 : 1, dst ), as P2ElementwiseOperator
   void apply( const P2Function< double >& src, const P2Function< double >& dst, uint_t level, const Selection& flag, UpdateType updateType = Replace ) const
   {
      gemv( 1.0, src, updateType == Replace ? 0.0 : 1.0, dst, level, flag );
   }
   // the schedule of P2ElementwiseOperator::gemv: every cell adds the contributions of its own micro-cells, the additive exchange
   // completes the shared DoFs; beta != 0 on several cells through a temporary
   void gemv( double alpha, const P2Function< double >& src, double beta, const P2Function< double >& dst, uint_t level, const Selection& flagIn ) const
   {
      if ( &src == &dst || &dst == &k_ )
         throw std::runtime_error( "P2ElementwiseDivKGrad::gemv: dst must differ from src and from k" );
      const Selection flag   = dst.effectiveFlag( flagIn ); // the destination's boundary condition decides; temporaries follow it
      const bool      shared = storage_->getCells().size() > 1;
      if ( !shared )
      {
         if ( beta != 0.0 && beta != 1.0 )
            dst.assign( { beta }, { dst }, level, flag );
         launch( alpha, src, dst, level, flag, beta == 0.0 ? HYTEG_HIP_REPLACE : HYTEG_HIP_ADD );
         return;
      }
      if ( beta == 0.0 )
      {
         launch( alpha, src, dst, level, flag, HYTEG_HIP_REPLACE );
         dst.getVertexDoFFunction().sumSharedCopies( level, flag );
         dst.sumSharedEdgeCopies( level, flag );
         return;
      }
      P2Function< double > tmp( "p2_divkgrad_gemv_tmp", storage_, level, level );
      launch( alpha, src, tmp, level, flag, HYTEG_HIP_REPLACE );
      tmp.getVertexDoFFunction().sumSharedCopies( level, flag );
      tmp.sumSharedEdgeCopies( level, flag );
      dst.assign( { beta, 1.0 }, { dst, tmp }, level, flag );
   }

   // per cell the diagonal kernel (every DoF: the sum of A_e[i][i] over this cell's micro-cells), the additive exchange, and the
   // reciprocal on the host (set-up time, once per operator), as P2ElementwiseOperator::computeInverseDiagonalOperatorValues
   void computeInverseDiagonalOperatorValues()
   {
      invDiag_.reset( new P2Function< double >( "inverse diagonal entries", storage_, minLevel_, maxLevel_ ) );
      const P2Function< double >& d = *invDiag_;
      for ( uint_t l = minLevel_; l <= maxLevel_; ++l )
      {
         for ( uint_t c = 0; c < storage_->getNumberOfLocalCells(); ++c )
            hipCheck( hyteg_hip_p2_elementwise_divkgrad_diagonal_cell( d.getVertexDoFFunction().getCellPointer( c, l ), d.getEdgeCellPointer( c, l ),
                                                                       k_.getVertexDoFFunction().getCellPointer( c, l ), k_.getEdgeCellPointer( c, l ), (int) l,
                                                                       geometry_.at( l ).at( c ).data(), storage_->stream() ),
                      "P2ElementwiseDivKGrad: diagonal" );
         if ( storage_->getCells().size() > 1 )
         {
            d.getVertexDoFFunction().sumSharedCopies( l, All );
            d.sumSharedEdgeCopies( l, All );
         }
         invertElementwise( d, l );
      }
   }
   std::shared_ptr< P2Function< double > > getInverseDiagonalValues() const
   {
      if ( !invDiag_ )
         throw std::runtime_error( "Inverse diagonal values have not been assembled, call computeInverseDiagonalOperatorValues() "
                                   "to set up this function." );
      return invDiag_;
   }

   // P2ElementwiseOperator::smooth_jac (P2ElementwiseOperator.cpp:344-374), statement by statement:
   //   dst = A src;  dst = rhs - dst;  dst = D^-1 dst;  dst = src + relax dst
   void smooth_jac( const P2Function< double >& dst, const P2Function< double >& rhs, const P2Function< double >& src, double relax, uint_t level,
                    const Selection& flag ) const
   {
      if ( &dst == &src )
         throw std::runtime_error( "P2ElementwiseDivKGrad::smooth_jac: src and dst must differ" );
      apply( src, dst, level, flag );
      dst.assign( { 1.0, -1.0 }, { rhs, dst }, level, flag );
      dst.multElementwise( { *getInverseDiagonalValues(), dst }, level, flag );
      dst.assign( { 1.0, relax }, { src, dst }, level, flag );
   }

 private:
   void launch( double alpha, const P2Function< double >& src, const P2Function< double >& dst, uint_t level, const Selection& flag, int update ) const
   {
      const std::vector< unsigned > masks = storage_->masksFor( flag, false, HYTEG_HIP_MASK_ALL );
      for ( uint_t c = 0; c < storage_->getNumberOfLocalCells(); ++c )
         hipCheck( hyteg_hip_p2_elementwise_divkgrad_apply_cell_kinds(
                       dst.getVertexDoFFunction().getCellPointer( c, level ), dst.getEdgeCellPointer( c, level ),
                       src.getVertexDoFFunction().getCellPointer( c, level ), src.getEdgeCellPointer( c, level ),
                       k_.getVertexDoFFunction().getCellPointer( c, level ), k_.getEdgeCellPointer( c, level ), (int) level,
                       geometry_.at( level ).at( c ).data(), alpha, update, masks[c], 0xFFu, storage_->stream() ),
                   "P2ElementwiseDivKGrad::gemv" );
   }

   std::shared_ptr< PrimitiveStorage >                          storage_;
   uint_t                                                       minLevel_, maxLevel_;
   const P2Function< double >&                                  k_;
   std::map< uint_t, std::vector< std::array< double, 60 > > >  geometry_; // per level and local cell
   uint64_t                                                     uid_ = nextUid();
   std::shared_ptr< P2Function< double > >                      invDiag_;
};

} // namespace operatorgeneration
} // namespace hyteg
