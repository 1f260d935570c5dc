// p2divkgrad.hpp -- part of the C++ host layer above the C-ABI (see hyteg_host.hpp for the data model).
// P2ElementwiseDivKGrad: the generated variable-coefficient diffusion operator -div( k grad u ) on P2 with a P2 coefficient function,
//    operatorgeneration::P2ElementwiseDivKGrad( storage, minLevel, maxLevel, const P2Function< real_t >& k )
// (module hyteg_operators; call site and known answer: tests/hyteg/convergence/ElementwiseDivKGradCGConvergenceTest.cpp:192-221), and
// forms::P2MassForm, the form of P2ElementwiseMassOperator (P2ElementwiseOperator.hpp) that the known-answer test builds its right-hand
// side with.  The operator has the interface and the schedules of P2ElementwiseOperator (p2operator.hpp): per cell the C-ABI seam
// hyteg_hip_p2_elementwise_divkgrad_apply_cell_kinds, then the additive exchange of the shares of the shared DoFs.  The operator at
// level l reads k at level l: the caller interpolates k on every level it uses, as the reference test does.  No smooth_sor, no constant
// stencils.  The operator offers what GeometricMultigridSolver and ChebyshevSmoother look for (residual, chebyshevStart / Step /
// Finish) and a fused smooth_jac: one launch per step and cell (hyteg_hip_p2_elementwise_divkgrad_*_cell, schedule: p2varcoefsteps.hpp).
#pragma once

#include "p2operator.hpp"
#include "p2varcoefsteps.hpp"

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

   // the fused Jacobi, residual and Chebyshev entries (default), or the composed passes everywhere (tests, measurements)
   void setFused( bool on ) { fused_ = on; }
   bool getFused() const { return fused_; }

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
   // Fused: the four statements in the epilogue of the apply kernels (hyteg_hip_p2_elementwise_divkgrad_jacobi_cell)
   void smooth_jac( const P2Function< double >& dst, const P2Function< double >& rhs, const P2Function< double >& src, double relax, uint_t level,
                    const Selection& flag ) const
   {
      if ( &dst == &src )
         throw std::runtime_error( "P2ElementwiseDivKGrad::smooth_jac: src and dst must differ" );
      const auto& invDiag = *getInverseDiagonalValues();
      if ( fused_ && &dst != &rhs && &dst != &invDiag && &dst != &k_ )
      {
         step( p2varcoef::Step::Jacobi, { { &dst }, { &src }, { &rhs }, { &invDiag }, { nullptr } }, dst.effectiveFlag( flag ), level, relax, 0.0, false );
         return;
      }
      apply( src, dst, level, flag );
      dst.assign( { 1.0, -1.0 }, { rhs, dst }, level, flag );
      dst.multElementwise( { invDiag, dst }, level, flag );
      dst.assign( { 1.0, relax }, { src, dst }, level, flag );
   }

   // r = b - A x as the multigrid cycle writes it (GeometricMultigridSolver.hpp:240-246: apply, then assign).  Fused: one launch per cell
   // (hyteg_hip_p2_elementwise_divkgrad_residual_cell); composed where r is x or b, and with setFused( false )
   void residual( const P2Function< double >& x, const P2Function< double >& b, const P2Function< double >& r, uint_t level, const Selection& flag ) const
   {
      if ( !fused_ || &r == &x || &r == &b )
      {
         apply( x, r, level, flag );
         r.assign( { 1.0, -1.0 }, { b, r }, level, flag );
         return;
      }
      step( p2varcoef::Step::Residual, { { &r }, { &x }, { &b }, { nullptr }, { nullptr } }, r.effectiveFlag( flag ), level, 0.0, 0.0, false );
   }

   // ---- the steps of ChebyshevSmoother::solve (ChebyshevSmoother.hpp:165-212) with the semantics of P1ConstantOperator's
   // (p1operator.hpp): one launch per step and cell (hyteg_hip_p2_elementwise_divkgrad_chebyshev_*_cell).  Where chebyshevFusable is
   // false the smoother runs its generic sequence.
   bool chebyshevFusable( uint_t ) const { return fused_; }
   // t = invDiag .* ( b - A x ); on the shell of several cells also x += c0 t.  Elsewhere x is this launch's source: its update is carried
   // out by the following chebyshevStep( ..., hasPrev = true ) or by chebyshevFinish
   void chebyshevStart( const P2Function< double >& t, const P2Function< double >& b, const P2Function< double >& x, double c0, uint_t level,
                        const Selection& flag ) const
   {
      const auto& invDiag = *getInverseDiagonalValues();
      checkOutput( "chebyshevStart", t, { &b, &x, &invDiag } );
      step( p2varcoef::Step::ChebStart, { { &t }, { &x }, { &b }, { &invDiag }, { &x } }, x.effectiveFlag( flag ), level, c0, 0.0, false );
   }
   // tOut = invDiag .* ( A tIn ); x = ( x + cPrev tIn ) + cCur tOut (first term only if hasPrev: the update chebyshevStart left open); on the
   // shell of several cells x += cCur tOut
   void chebyshevStep( const P2Function< double >& tOut, const P2Function< double >& x, const P2Function< double >& tIn, double cPrev, double cCur,
                       bool hasPrev, uint_t level, const Selection& flag ) const
   {
      const auto& invDiag = *getInverseDiagonalValues();
      checkOutput( "chebyshevStep", tOut, { &x, &tIn, &invDiag } );
      checkOutput( "chebyshevStep", x, { &tIn, &invDiag } );
      step( p2varcoef::Step::ChebStep, { { &tOut }, { &tIn }, { nullptr }, { &invDiag }, { &x } }, x.effectiveFlag( flag ), level, cCur, cPrev, hasPrev );
   }
   // x += c t where the start deferred it: closes a smoother call of order 1 (no step follows the start)
   void chebyshevFinish( const P2Function< double >& x, const P2Function< double >& t, double c, uint_t level, const Selection& flag ) const
   {
      p2varcoef::chebyshevFinish< 1 >( storage_, { &x }, { &t }, { x.effectiveFlag( flag ) }, c, level );
   }

 private:
   void checkOutput( const char* who, const P2Function< double >& out, std::initializer_list< const P2Function< double >* > inputs ) const
   {
      bool bad = &out == &k_;
      for ( const P2Function< double >* f : inputs )
         bad = bad || &out == f;
      if ( bad )
         throw std::runtime_error( std::string( "P2ElementwiseDivKGrad::" ) + who + ": an output must differ from the inputs and from k" );
   }
   // one fused step (p2varcoefsteps.hpp): a = relax, c0 or cCur
   void step( p2varcoef::Step what, const p2varcoef::Operands< 1 >& f, const Selection& flag, uint_t level, double a, double cPrev, bool hasPrev ) const
   {
      p2varcoef::fusedStep< 1 >(
          storage_, what, f, { flag }, level, a, [&] { launch( 1.0, *f.src[0], *f.out[0], level, flag, HYTEG_HIP_REPLACE, HYTEG_HIP_MASK_SHELL ); },
          [&]( uint_t c, const std::array< unsigned, 1 >& m ) {
             const auto v = [&]( const P2Function< double >* g ) -> double* { return g ? g->getVertexDoFFunction().getCellPointer( c, level ) : nullptr; };
             const auto e = [&]( const P2Function< double >* g ) -> double* { return g ? g->getEdgeCellPointer( c, level ) : nullptr; };
             const double *kv = v( &k_ ), *ke = e( &k_ ), *geo = geometry_.at( level ).at( c ).data();
             const int     l = (int) level;
             hyteg_hip_stream_t s  = storage_->stream();
             int         rc = 0;
             switch ( what )
             {
             case p2varcoef::Step::Residual:
                rc = hyteg_hip_p2_elementwise_divkgrad_residual_cell( v( f.out[0] ), e( f.out[0] ), v( f.src[0] ), e( f.src[0] ), v( f.rhs[0] ), e( f.rhs[0] ), kv, ke,
                                                                      l, geo, m[0], 0xFFu, s );
                break;
             case p2varcoef::Step::Jacobi:
                rc = hyteg_hip_p2_elementwise_divkgrad_jacobi_cell( v( f.out[0] ), e( f.out[0] ), v( f.src[0] ), e( f.src[0] ), v( f.rhs[0] ), e( f.rhs[0] ),
                                                                    v( f.inv[0] ), e( f.inv[0] ), kv, ke, l, geo, a, m[0], 0xFFu, s );
                break;
             case p2varcoef::Step::ChebStart:
                rc = hyteg_hip_p2_elementwise_divkgrad_chebyshev_start_cell( v( f.out[0] ), e( f.out[0] ), v( f.src[0] ), e( f.src[0] ), v( f.rhs[0] ),
                                                                             e( f.rhs[0] ), v( f.inv[0] ), e( f.inv[0] ), kv, ke, l, geo, m[0], 0xFFu, s );
                break;
             case p2varcoef::Step::ChebStep:
                rc = hyteg_hip_p2_elementwise_divkgrad_chebyshev_step_cell( v( f.out[0] ), e( f.out[0] ), v( f.x[0] ), e( f.x[0] ), v( f.src[0] ), e( f.src[0] ),
                                                                            v( f.inv[0] ), e( f.inv[0] ), kv, ke, l, geo, cPrev, a, hasPrev ? 1 : 0, m[0], 0xFFu, s );
                break;
             }
             hipCheck( rc, "P2ElementwiseDivKGrad: fused step" );
          } );
   }
   void launch( double alpha, const P2Function< double >& src, const P2Function< double >& dst, uint_t level, const Selection& flag, int update,
                unsigned keep = HYTEG_HIP_MASK_ALL ) const
   {
      const std::vector< unsigned > masks = storage_->masksFor( flag, false, keep );
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
   bool                                                         fused_ = true;
};

} // namespace operatorgeneration
} // namespace hyteg
