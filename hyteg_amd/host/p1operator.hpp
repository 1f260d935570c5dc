// p1operator.hpp -- part of the C++ host layer above the C-ABI (see hyteg_host.hpp for the data model).
// P1ConstantOperator< Form > (src/constant_stencil_operator/P1ConstantOperator.hpp,
// src/hyteg/p1functionspace/P1Operator.hpp)
#pragma once

#include "forms.hpp"
#include "p1function.hpp"

namespace hyteg {

// =====================================================================================================
// P1ConstantOperator< Form >  ( src/constant_stencil_operator/P1ConstantOperator.hpp:33-168 )
// =====================================================================================================
template < class Form >
class P1ConstantOperator
{
 public:
   using srcType = P1Function< double >;
   using dstType = P1Function< double >;
   using FunctionList = std::vector< std::reference_wrapper< const P1Function< double > > >;

   P1ConstantOperator( const std::shared_ptr< PrimitiveStorage >& storage, uint_t minLevel, uint_t maxLevel )
   : storage_( storage )
   , minLevel_( minLevel )
   , maxLevel_( maxLevel )
   {
      storage->markInUse(); // the mesh boundary flags are fixed from here on
      // assembleStencils(), P1ConstantOperator.cpp:680-732: per level and cell
      for ( uint_t l = minLevel; l <= maxLevel; ++l )
      {
         std::vector< stencil::CellStencils > perCell;
         for ( const auto& cell : storage->getCells() ) // all cells: inverse diagonals need the neighbours' shares
            perCell.push_back( stencil::assemble< Form >( cell, l ) );
         stencils_[l] = perCell;
         sorTables_[l] = buildSorTables( perCell );
         if ( l >= HYTEG_HIP_MIN_LEVEL )
            hipCheck( hyteg_hip_prepare_level( (int) l ), "P1ConstantOperator: prepare_level" );
      }
   }

   std::shared_ptr< PrimitiveStorage > getStorage() const { return storage_; }
   uint64_t                            uid() const { return uid_; }
   uint_t                              getMinLevel() const { return minLevel_; }
   uint_t                              getMaxLevel() const { return maxLevel_; }
   const stencil::CellStencils&        getCellStencils( int globalCellID, uint_t level ) const { return stencils_.at( level ).at( globalCellID ); }

   // Operator::apply, P1Operator.hpp:192-320
   void apply( const P1Function< double >& src, const P1Function< double >& dst, uint_t level, const Selection& flagIn, UpdateType updateType = Replace ) const
   {
      ScopedTimer timerOp( storage_->getTimingTree(), "Operator P1Function to P1Function" ), timerApply( storage_->getTimingTree(), "Apply" );
      const Selection flag = dst.effectiveFlag( flagIn ); // the function's boundary condition decides what `Inner` means
      if ( &src == &dst )
         throw std::runtime_error( "P1ConstantOperator::apply: src and dst must differ (P1Operator.hpp:198)" );
      if ( storage_->lanesOpen() )
      {
         // inside a lane scope (the loop of apply_cycle): an apply that consists of interior launches only -- each reads src's
         // cell array and writes dst's -- goes where the planner puts it, next to the applies it does not depend on; every
         // other apply runs behind all lanes, as ever
         if ( pureInterior( level, flag ) )
         {
            storage_->forLocalCells( [&]( uint_t c, const MacroCell& cell ) {
               if ( !( storage_->maskFor( cell, flag ) & HYTEG_HIP_MASK_INNER ) )
                  return;
               double*            d    = dst.getCellPointer( c, level );
               const double*      u    = src.getCellPointer( c, level );
               const void*        r[1] = { u };
               const void*        w[1] = { d };
               hyteg_hip_stream_t lane = storage_->laneFor( r, 1, w, 1 );
               hipCheck( hyteg_hip_p1_apply_cell( d, u, (int) level, getCellStencils( cell.id, level ).inner, hipUpdate( updateType ), lane ),
                         "apply: cell" );
            } );
            return;
         }
         storage_->joinLanes();
      }
      if ( storage_->useBatch( level ) )
      {
         applyBatched( src, dst, level, flag, updateType );
         return;
      }
      // partial results of shared DoFs are summed over cells before they are added to dst
      std::unique_ptr< P1Function< double > > tmp;
      if ( updateType == Add && hasSharedPoints( level, flag ) )
         tmp = P1Function< double >::zeroedScratch( "apply_tmp", storage_, level );
      const P1Function< double >& shellDst    = tmp ? *tmp : dst;
      const int                   shellUpdate = hipUpdate( tmp ? Replace : updateType );
      // 1. this cell's share of the shared macro-face/edge/vertex DoFs (tiny kernels), 2. start the halo exchange,
      // 3. the interior stencil while the exchange is in flight, 4. reduce the shares.  1, 2 and 4 only touch shared points:
      // with a stream-agnostic transport they can form a chain on a side stream next to 3 (PrimitiveStorage::SideChain;
      // opt-in, measured slower than one stream).
      const bool                  sideChain = storage_->sideChainUsable( (int) level, flag, 0 );
      PrimitiveStorage::SideChain chain( *storage_, sideChain );
      // the interiors of the cells are independent launches: with enough cells they alternate between the lanes of the storage
      // (one fork behind the shell kernels, one join in front of the reduction of the shares), see PrimitiveStorage::applyCellLanesMin()
      PrimitiveStorage::LaneScope cellLanes( *storage_, !sideChain && storage_->applyCellLanesMin() > 0 && storage_->getNumberOfLocalCells() >= storage_->applyCellLanesMin() &&
                                                            level >= HYTEG_HIP_MIN_LEVEL );
      // a rank with ONE macro-cell that exchanges peer to peer: the share kernel stores the shares into the peers' slots itself
      PrimitiveStorage::ShareSend send;
      const bool bySharesKernel = shellDst.beginSumSharedCopiesByShares( level, flag, send );
      storage_->forLocalCells( [&]( uint_t c, const MacroCell& cell ) {
         const auto& S = getCellStencils( cell.id, level );
         if ( bySharesKernel )
         {
            hipCheck( hyteg_hip_p1_apply_cell_boundary_p2p( shellDst.getCellPointer( c, level ), src.getCellPointer( c, level ), (int) level,
                                                            &S.slots[0][0], storage_->maskFor( cell, flag ), shellUpdate, send.first, send.list,
                                                            send.a.peers, send.a.npeers, send.a.seq, send.a.counter, storage_->stream() ),
                      "apply: boundary + send" );
            return;
         }
         hipCheck( hyteg_hip_p1_apply_cell_boundary( shellDst.getCellPointer( c, level ), src.getCellPointer( c, level ), (int) level,
                                                     &S.slots[0][0], storage_->maskFor( cell, flag ), shellUpdate, storage_->stream() ),
                   "apply: boundary" );
      } );
      if ( !bySharesKernel )
         shellDst.beginSumSharedCopies( level, flag );
      chain.toMain();
      storage_->forLocalCells( [&]( uint_t c, const MacroCell& cell ) {
         const unsigned mask = storage_->maskFor( cell, flag );
         if ( ( mask & HYTEG_HIP_MASK_INNER ) && level >= HYTEG_HIP_MIN_LEVEL )
            hipCheck( hyteg_hip_p1_apply_cell( dst.getCellPointer( c, level ), src.getCellPointer( c, level ), (int) level,
                                               getCellStencils( cell.id, level ).inner, hipUpdate( updateType ),
                                               // the first cell on lane 1: forked before any interior is on the storage's stream
                                               cellLanes.active() ? storage_->laneStream( (int) c + 1 ) : storage_->stream() ),
                      "apply: cell" );
      } );
      cellLanes.join();
      chain.toSide();
      shellDst.endSumSharedCopies( level, flag );
      chain.join();
      if ( tmp )
         dst.addOnShell( *tmp, level, flag );
   }

   // A run of applies the caller sees as a whole before it issues the first (the loop of apply_cycle): step k is
   // apply( *srcs[k], *dsts[k], level, flag, updateType ), with the same results.  Where every step is one interior launch on the
   // one local macro-cell, consecutive independent steps share a launch (hyteg_hip_p1_apply_cell_steps; groups from planApplySteps,
   // up to PrimitiveStorage::applySteps() steps each): the grid of a group carries the bricks of all its steps, so a step starts
   // while the waves of the one before it drain, with no kernel boundary in between.  A group is placed on the storage's lanes like
   // a single apply that reads all its sources and writes all its destinations, and is sized so that every lane still gets one.
   // Anything else is the plain loop.
   void applyRun( const std::vector< const P1Function< double >* >& srcs, const std::vector< const P1Function< double >* >& dsts, uint_t level,
                  const Selection& flagIn, UpdateType updateType = Replace ) const
   {
      const int n       = (int) srcs.size();
      const int G       = storage_->applySteps();
      storage_->resetStepsLaunches();
      // up to level 8: a level-9 launch is 70 us of several generations of waves, groups gain nothing there (measured: 70.7 -> 70.5-71.4 us)
      bool      grouped = G > 1 && n > 1 && level <= 8 && storage_->getNumberOfLocalCells() == 1 && storage_->applyStepsUsable();
      for ( int k = 0; k < n && grouped; ++k )
      {
         const Selection flag = dsts[k]->effectiveFlag( flagIn );
         grouped            = srcs[k] != dsts[k] && pureInterior( level, flag );
         storage_->forLocalCells( [&]( uint_t, const MacroCell& cell ) { grouped = grouped && ( storage_->maskFor( cell, flag ) & HYTEG_HIP_MASK_INNER ); } );
      }
      if ( !grouped )
      {
         for ( int k = 0; k < n; ++k )
            apply( *srcs[k], *dsts[k], level, flagIn, updateType );
         return;
      }
      std::vector< const void* > u( (size_t) n );
      std::vector< void* >       d( (size_t) n );
      const double*              stencil = nullptr;
      storage_->forLocalCells( [&]( uint_t c, const MacroCell& cell ) {
         stencil = getCellStencils( cell.id, level ).inner;
         for ( int k = 0; k < n; ++k )
         {
            u[(size_t) k] = srcs[k]->getCellPointer( c, level );
            d[(size_t) k] = dsts[k]->getCellPointer( c, level );
         }
      } );
      const int upd = hipUpdate( updateType );
      int       k   = 0;
      for ( const int g : planApplySteps( u.data(), d.data(), n, G, storage_->lanesOpen() ? storage_->applyLanes() : 1 ) )
      {
         const void* const* r = u.data() + k;
         void* const*       w = d.data() + k;
         hyteg_hip_stream_t s = storage_->lanesOpen() ? storage_->laneFor( r, g, w, g ) : storage_->stream();
         int                rc = g > 1 ? hyteg_hip_p1_apply_cell_steps( w, r, g, (int) level, stencil, upd, s ) : HYTEG_HIP_ENOTSUP;
         if ( g > 1 && rc == HYTEG_HIP_OK )
            storage_->countStepsLaunch();
         if ( rc == HYTEG_HIP_ENOTSUP ) // a group of one, or a level without a steps kernel: one by one on the same stream
         {
            rc = HYTEG_HIP_OK;
            for ( int i = 0; i < g && rc == HYTEG_HIP_OK; ++i )
               rc = hyteg_hip_p1_apply_cell( static_cast< double* >( w[i] ), static_cast< const double* >( r[i] ), (int) level, stencil, upd, s );
         }
         hipCheck( rc, "applyRun: cell" );
         k += g;
      }
   }

   // r = b - A x on the points `flag` selects: apply followed by assign( { 1, -1 }, { b, r } ) as the multigrid cycle writes it
   // (GeometricMultigridSolver.hpp:240-246); where no shell point is selected (one macro-cell with fixed boundary values) the
   // interior kernel forms the difference itself -- one launch, the same bits
   void residual( const P1Function< double >& x, const P1Function< double >& b, const P1Function< double >& r, uint_t level, const Selection& flagIn ) const
   {
      const Selection flag = r.effectiveFlag( flagIn );
      if ( !pureInterior( level, flag ) || level > 10 || &x == &r )
      {
         apply( x, r, level, flagIn );
         r.assign( { 1.0, -1.0 }, { b, r }, level, flagIn );
         return;
      }
      ScopedTimer timerOp( storage_->getTimingTree(), "Operator P1Function to P1Function" ), timerApply( storage_->getTimingTree(), "Apply" );
      storage_->forLocalCells( [&]( uint_t c, const MacroCell& cell ) {
         if ( storage_->maskFor( cell, flag ) & HYTEG_HIP_MASK_INNER )
            hipCheck( hyteg_hip_p1_residual_cell( r.getCellPointer( c, level ), b.getCellPointer( c, level ), x.getCellPointer( c, level ),
                                                  (int) level, getCellStencils( cell.id, level ).inner, storage_->stream() ),
                      "residual: cell" );
      } );
   }

   // P1Operator::smooth_jac, P1Operator.hpp:429-447
   void smooth_jac( const P1Function< double >& dst, const P1Function< double >& rhs, const P1Function< double >& src, double relax,
                    uint_t level, const Selection& flagIn ) const
   {
      ScopedTimer timerOp( storage_->getTimingTree(), "Operator P1Function to P1Function" ), timerJac( storage_->getTimingTree(), "smooth_jac" );
      const Selection flag = dst.effectiveFlag( flagIn ); // the function's boundary condition decides what `Inner` means
      if ( &src == &dst )
         throw std::runtime_error( "smooth_jac: src and dst must differ" );
      const auto& invDiag = *getInverseDiagonalValues();
      if ( storage_->useBatch( level ) )
      {
         // phase 0: inner points complete, shell points this cell's share; exchange; phase 1: shell update
         const auto masks = storage_->masksFor( flag );
         for ( int phase = 0; phase < 2; ++phase )
         {
            storage_->forCellChunks( [&]( int first, int count ) {
               const auto d = dst.cellPointers( level, first, count ), r = rhs.cellPointers( level, first, count ),
                          u = src.cellPointers( level, first, count ), iv = invDiag.cellPointers( level, first, count );
               hipCheck( hyteg_hip_p1_jacobi_cells( count, d.data(), r.data(), u.data(), iv.data(), (int) level,
                                                    stencilTable( level ) + (size_t) first * 225, relax, masks.data() + first, phase,
                                                    storage_->stream() ),
                         "smooth_jac (batched)" );
            } );
            if ( phase == 0 )
               dst.sumSharedCopies( level, flag );
         }
         return;
      }
      interiorsAndShares( dst, src, level, flag, [&]( uint_t c, const double* inner ) {
         if ( level >= HYTEG_HIP_MIN_LEVEL )
            hipCheck( hyteg_hip_p1_jacobi_cell( dst.getCellPointer( c, level ), rhs.getCellPointer( c, level ), src.getCellPointer( c, level ),
                                                nullptr, (int) level, inner, relax, storage_->stream() ),
                      "smooth_jac: cell" );
      } );
      // on the shell: dst = rhs - dst ; dst = invDiag .* dst ; dst = src + relax * dst  (the reference's three passes)
      shellPasses( dst, &rhs, invDiag, src, relax, dst, level, flag );
   }

   // ---- the steps of ChebyshevSmoother::solve (ChebyshevSmoother.hpp:165-212), fused like smooth_jac: one launch per step on
   // the interiors the mask selects (hyteg_hip_p1_chebyshev_{start,step}_cell, scalar inverse diagonal = what
   // computeInverseDiagonalOperatorValues stores there), this cell's shares of the shell points, sumSharedCopies, then the masked
   // vector kernels for invDiag .* and the update of x on the shell.  Used on the levels the storage does not batch (the batched
   // levels take the smoother's generic sequence, whose apply and vector kernels are one launch for all cells).
   bool chebyshevFusable( uint_t level ) const { return !storage_->useBatch( level ) && level >= HYTEG_HIP_MIN_LEVEL; }
   // t = invDiag .* ( b - A x ) on the selected points; on the shell also x += c0 t.  On the interiors x is this launch's stencil
   // source: its update x += c0 t is carried out by the following chebyshevStep( ..., hasPrev = true ) or by chebyshevFinish.
   void chebyshevStart( const P1Function< double >& t, const P1Function< double >& b, const P1Function< double >& x, double c0, uint_t level,
                        const Selection& flagIn ) const
   {
      ScopedTimer timerOp( storage_->getTimingTree(), "Operator P1Function to P1Function" ), timerCheb( storage_->getTimingTree(), "chebyshev" );
      const Selection flag = x.effectiveFlag( flagIn );
      if ( &t == &x || &t == &b )
         throw std::runtime_error( "chebyshevStart: t must differ from x and b" );
      interiorsAndShares( t, x, level, flag, [&]( uint_t c, const double* inner ) {
         hipCheck( hyteg_hip_p1_chebyshev_start_cell( t.getCellPointer( c, level ), b.getCellPointer( c, level ), x.getCellPointer( c, level ),
                                                      nullptr, (int) level, inner, storage_->stream() ),
                   "chebyshevStart: cell" );
      } );
      // on the shell: t = b - t ; t = invDiag .* t ; x = x + c0 t
      shellPasses( t, &b, *getInverseDiagonalValues(), x, c0, x, level, flag );
   }
   // tOut = invDiag .* ( A tIn ) on the selected points; x = ( x + cPrev tIn ) + cCur tOut on the interiors (first term only if
   // hasPrev: the update chebyshevStart left open), x += cCur tOut on the shell
   void chebyshevStep( const P1Function< double >& tOut, const P1Function< double >& x, const P1Function< double >& tIn, double cPrev, double cCur,
                       bool hasPrev, uint_t level, const Selection& flagIn ) const
   {
      ScopedTimer timerOp( storage_->getTimingTree(), "Operator P1Function to P1Function" ), timerCheb( storage_->getTimingTree(), "chebyshev" );
      const Selection flag = x.effectiveFlag( flagIn );
      if ( &tOut == &tIn || &tOut == &x || &x == &tIn )
         throw std::runtime_error( "chebyshevStep: tOut, x and tIn must be three different functions" );
      interiorsAndShares( tOut, tIn, level, flag, [&]( uint_t c, const double* inner ) {
         hipCheck( hyteg_hip_p1_chebyshev_step_cell( tOut.getCellPointer( c, level ), x.getCellPointer( c, level ), tIn.getCellPointer( c, level ),
                                                     nullptr, (int) level, inner, cPrev, cCur, hasPrev ? 1 : 0, storage_->stream() ),
                   "chebyshevStep: cell" );
      } );
      // on the shell: tOut = invDiag .* tOut ; x = x + cCur tOut
      shellPasses( tOut, nullptr, *getInverseDiagonalValues(), x, cCur, x, level, flag );
   }
   // x += c t on the interiors: closes a smoother call of order 1 (no step follows the start)
   void chebyshevFinish( const P1Function< double >& x, const P1Function< double >& t, double c, uint_t level, const Selection& flagIn ) const
   {
      const Selection flag = x.effectiveFlag( flagIn );
      storage_->forLocalCells( [&]( uint_t ci, const MacroCell& cell ) {
         const unsigned inner = storage_->maskFor( cell, flag ) & HYTEG_HIP_MASK_INNER;
         if ( !inner )
            return;
         double*       d     = x.getCellPointer( ci, level );
         const double* u[2]  = { d, t.getCellPointer( ci, level ) };
         const double  sc[2] = { 1.0, c };
         hipCheck( hyteg_hip_p1_vector_cell_masked( 0, d, 2, u, sc, (int) level, inner, storage_->stream() ), "chebyshevFinish" );
      } );
   }

   // `steps` consecutive sweeps of smooth_sor (what a multigrid cycle's pre- / post-smoothing loop does,
   // GeometricMultigridSolver.hpp:209-215).  Where no shared or boundary point is swept (every macro-cell's shell is fixed: one
   // macro-cell with Dirichlet values, or cells whose common faces are not selected by the flag) the sweeps of a cell do not
   // see anybody else's updates in between, and from level 5 on they run as one pipeline of block wavefronts
   // (hyteg_hip_p1_sor_cell_sweeps: bit-identical to the loop, 46 + 4 ( steps - 1 ) launches instead of 46 steps at level 8).
   void smooth_sor_steps( const P1Function< double >& dst, const P1Function< double >& rhs, double relax, uint_t level, const Selection& flagIn,
                          uint_t steps, bool backwards = false ) const
   {
      const Selection flag = dst.effectiveFlag( flagIn );
      if ( steps <= 1 || storage_->anyShellSelected( flag ) || storage_->numRanks() != 1 || storage_->useBatchSor( level ) || level < 5 )
      {
         for ( uint_t k = 0; k < steps; ++k )
            smooth_sor( dst, rhs, relax, level, flagIn, backwards );
         return;
      }
      ScopedTimer timerOp( storage_->getTimingTree(), "Operator P1Function to P1Function" ), timerSor( storage_->getTimingTree(), backwards ? "SOR backwards" : "SOR" );
      if ( &dst == &rhs )
         throw std::runtime_error( "smooth_sor: dst and rhs must differ" );
      storage_->forLocalCells( [&]( uint_t c, const MacroCell& cell ) {
         if ( storage_->maskFor( cell, flag ) & HYTEG_HIP_MASK_INNER )
            hipCheck( hyteg_hip_p1_sor_cell_sweeps( dst.getCellPointer( c, level ), rhs.getCellPointer( c, level ), (int) level,
                                                    getCellStencils( cell.id, level ).inner, relax, backwards ? 1 : 0, (int) steps,
                                                    storage_->stream() ),
                      "smooth_sor_steps: cell" );
      } );
   }
   // P1Operator::smooth_sor / smooth_gs, P1Operator.hpp:322-418: macro-vertices, -edges, -faces, -cells (reversed for
   // backwards), each class with the values the reference's communication schedule gives it.  Cell-centric form:
   //  rest  = (stencil sum over the neighbours outside the primitive's closure), summed over cells by ONE exchange,
   //          taken from the pre-sweep state (forward) -- the reference's ghost layers are not refreshed in between;
   //  sweep = every cell runs the vertex / edge / face sweeps on its own copies with the total weights (bit-identical
   //          copies, no further exchange), then the lexicographic macro-cell sweep.
   // Backwards the reference communicates before every class, so `rest` is rebuilt (and exchanged) per class.
   void smooth_sor( const P1Function< double >& dst, const P1Function< double >& rhs, double relax, uint_t level, const Selection& flagIn,
                    bool backwards = false ) const
   {
      if ( &dst == &rhs )
         throw std::runtime_error( "smooth_sor: dst and rhs must differ" );
      sorSchedule( { dst }, { rhs }, relax, level, dst.effectiveFlag( flagIn ), backwards );
   }
   // Several functions swept by the SAME launches (no counterpart in the reference, which sweeps one function at a time): the
   // Gauss-Seidel phases are chains of small dependent kernels whose duration does not depend on how many cells a launch
   // covers, and the batched kernels take any list of cell arrays -- so the three velocity components of the Stokes smoother
   // (StokesVelocityBlockBlockDiagonalPreconditioner) share one chain instead of running three.  The batch is ordered
   // [function][cell]; every function sees exactly the kernels, tables and order of smooth_sor: results are bit-identical.
   // Falls back to one smooth_sor per function where the batched path does not apply (large levels, different boundary
   // conditions).
   void smooth_sor_many( const FunctionList& dsts, const FunctionList& rhss, double relax, uint_t level, const Selection& flagIn, bool backwards = false ) const
   {
      const uint_t nf = dsts.size();
      if ( nf == 0 || rhss.size() != nf )
         throw std::runtime_error( "smooth_sor_many: need as many right-hand sides as functions" );
      const Selection flag     = dsts[0].get().effectiveFlag( flagIn );
      bool          together = nf > 1 && storage_->useBatch( level ) && storage_->useBatchSor( level );
      for ( uint_t k = 0; k < nf; ++k )
         together = together && dsts[k].get().effectiveFlag( flagIn ) == flag && &dsts[k].get() != &rhss[k].get();
      if ( together )
         sorSchedule( dsts, rhss, relax, level, flag, backwards );
      else
         for ( uint_t k = 0; k < nf; ++k )
            smooth_sor( dsts[k].get(), rhss[k].get(), relax, level, flagIn, backwards );
   }
   // The two halves of smooth_sor for callers that provide the stencil sum over the neighbours outside a primitive's closure
   // themselves (P2 operators: the vertex-to-vertex sweeps of P2ConstantOperator::smooth_sor_macro_{vertices,edges,faces,cells}
   // see the edge DoFs as well): the sweeps of the point classes in `bits` on every cell's copies with the total weights, `rest`
   // already summed over the cells; and the lexicographic macro-cell sweeps.
   void smooth_sor_shell_given_rest( const P1Function< double >& dst, const P1Function< double >& rhs, const P1Function< double >& rest,
                                     double relax, uint_t level, const Selection& flagIn, unsigned bits, bool backwards = false ) const
   {
      launchSorShell( { dst }, { rhs }, { rest }, relax, level, dst.effectiveFlag( flagIn ), bits, backwards );
   }
   void smooth_sor_cells_only( const P1Function< double >& dst, const P1Function< double >& rhs, double relax, uint_t level, const Selection& flagIn,
                               bool backwards = false ) const
   {
      launchSorCells( { dst }, { rhs }, relax, level, dst.effectiveFlag( flagIn ), backwards );
   }

 private:
   // the skeleton of a fused smoother step on the per-cell kernels: `interior( c, inner stencil )` launches the step on the
   // interior of every cell where the flag selects it, every cell's share of A src on the shell points goes to dst and the
   // shares are summed over the cells
   template < typename Interior >
   void interiorsAndShares( const P1Function< double >& dst, const P1Function< double >& src, uint_t level, const Selection& flag, Interior&& interior ) const
   {
      storage_->forLocalCells( [&]( uint_t c, const MacroCell& cell ) {
         const auto&    S    = getCellStencils( cell.id, level );
         const unsigned mask = storage_->maskFor( cell, flag );
         if ( mask & HYTEG_HIP_MASK_INNER )
            interior( c, S.inner );
         hipCheck( hyteg_hip_p1_apply_cell_boundary( dst.getCellPointer( c, level ), src.getCellPointer( c, level ), (int) level, &S.slots[0][0], mask,
                                                     HYTEG_HIP_REPLACE, storage_->stream() ),
                   "smoother step: boundary" );
      } );
      dst.sumSharedCopies( level, flag );
   }
   // the reference's passes on the shell points, after the shares of a stencil sum have been summed into t: t = rhs - t (if rhs),
   // t = invDiag .* t, out = base + c t -- operands in the reference's order
   void shellPasses( const P1Function< double >& t, const P1Function< double >* rhs, const P1Function< double >& invDiag,
                     const P1Function< double >& base, double c, const P1Function< double >& out, uint_t level, const Selection& flag ) const
   {
      storage_->forLocalCells( [&]( uint_t ci, const MacroCell& cell ) {
         const unsigned shell = storage_->maskFor( cell, flag ) & HYTEG_HIP_MASK_SHELL;
         if ( !shell )
            return;
         double* d = t.getCellPointer( ci, level );
         if ( rhs )
         {
            const double* a[2]  = { rhs->getCellPointer( ci, level ), d };
            const double  s1[2] = { 1.0, -1.0 };
            hipCheck( hyteg_hip_p1_vector_cell_masked( 0, d, 2, a, s1, (int) level, shell, storage_->stream() ), "shell passes: residual" );
         }
         const double* m[2] = { invDiag.getCellPointer( ci, level ), d };
         hipCheck( hyteg_hip_p1_vector_cell_masked( 2, d, 2, m, nullptr, (int) level, shell, storage_->stream() ), "shell passes: scale" );
         const double* u[2]  = { base.getCellPointer( ci, level ), d };
         const double  s2[2] = { 1.0, c };
         hipCheck( hyteg_hip_p1_vector_cell_masked( 0, out.getCellPointer( ci, level ), 2, u, s2, (int) level, shell, storage_->stream() ),
                   "shell passes: update" );
      } );
   }

   // ---- smooth_sor for the functions of a list at once: the order of the classes, once.  Each of the three stages below is
   // one launch per chunk of the list [function][cell] ([cell] for one function) where the storage batches the sweeps
   // (useBatchSor), else one launch per function and cell. ----
   void sorSchedule( const FunctionList& dsts, const FunctionList& rhss, double relax, uint_t level, const Selection& flag, bool backwards ) const
   {
      ScopedTimer timerOp( storage_->getTimingTree(), "Operator P1Function to P1Function" ), timerSor( storage_->getTimingTree(), backwards ? "SOR backwards" : "SOR" );
      auto sweepCells = [&]() { launchSorCells( dsts, rhss, relax, level, flag, backwards ); };
      if ( !storage_->anyShellSelected( flag ) && storage_->numRanks() == 1 )
      {
         sweepCells();
         return;
      }
      FunctionList rests;
      for ( uint_t k = 0; k < dsts.size(); ++k )
      {
         auto& slot = sorRest_[std::make_pair( level, k )];
         if ( !slot )
            slot.reset( new P1Function< double >( "sor_rest", storage_, level, level ) );
         rests.push_back( std::cref( *slot ) );
      }
      auto sweepShell = [&]( unsigned bits ) {
         launchSorRest( rests, dsts, level, flag, bits );
         launchSorShell( dsts, rhss, rests, relax, level, flag, bits, backwards );
      };
      if ( !backwards )
      {
         sweepShell( HYTEG_HIP_MASK_SHELL );
         sweepCells();
      }
      else
      {
         sweepCells();
         sweepShell( 0xFu << 6 );  // macro-faces
         sweepShell( 0x3Fu );      // macro-edges
         sweepShell( 0xFu << 10 ); // macro-vertices
      }
   }
   // calls fn( first, count ) for chunks of at most HYTEG_HIP_MAX_BATCH entries of the list [function][cell]
   template < typename F >
   void forBatchChunks( uint_t nf, F&& fn ) const
   {
      const int total = (int) ( nf * storage_->getNumberOfLocalCells() );
      for ( int first = 0; first < total; first += HYTEG_HIP_MAX_BATCH )
         fn( first, std::min( HYTEG_HIP_MAX_BATCH, total - first ) );
   }
   std::vector< double* > batchPointers( const FunctionList& fs, uint_t level, int first, int count ) const
   {
      const int              nc = (int) storage_->getNumberOfLocalCells();
      std::vector< double* > p;
      for ( int e = first; e < first + count; ++e )
         p.push_back( fs[(uint_t) ( e / nc )].get().getCellPointer( (uint_t) ( e % nc ), level ) );
      return p;
   }
   std::vector< unsigned > batchMasks( uint_t nf, const Selection& flag, unsigned keep ) const
   {
      const auto              once = storage_->masksFor( flag, false, keep );
      std::vector< unsigned > m;
      for ( uint_t k = 0; k < nf; ++k )
         m.insert( m.end(), once.begin(), once.end() );
      return m;
   }
   // rest = stencil sum over the neighbours outside the closure of the primitives of the classes in `bits`, summed over the cells
   void launchSorRest( const FunctionList& rests, const FunctionList& dsts, uint_t level, const Selection& flag, unsigned bits ) const
   {
      const uint_t nf = dsts.size();
      if ( storage_->useBatchSor( level ) )
      {
         const auto    masks = batchMasks( nf, flag, bits & HYTEG_HIP_MASK_SHELL );
         const double* table = restTable( level, nf );
         forBatchChunks( nf, [&]( int first, int count ) {
            const auto r = batchPointers( rests, level, first, count ), u = batchPointers( dsts, level, first, count );
            hipCheck( hyteg_hip_p1_apply_cells( count, r.data(), u.data(), (int) level, table + (size_t) first * 225, masks.data() + first,
                                                HYTEG_HIP_REPLACE, storage_->stream() ),
                      "smooth_sor: rest (batched)" );
         } );
      }
      else
         for ( uint_t k = 0; k < nf; ++k )
            storage_->forLocalCells( [&]( uint_t c, const MacroCell& cell ) {
               const auto&    T    = sorTables_.at( level ).at( cell.id );
               const unsigned mask = storage_->maskFor( cell, flag ) & bits;
               hipCheck( hyteg_hip_p1_apply_cell_boundary( rests[k].get().getCellPointer( c, level ), dsts[k].get().getCellPointer( c, level ),
                                                           (int) level, &T.rest[0][0], mask, HYTEG_HIP_REPLACE, storage_->stream() ),
                         "smooth_sor: rest" );
            } );
      for ( uint_t k = 0; k < nf; ++k )
         rests[k].get().sumSharedCopies( level, flag );
   }
   void launchSorCells( const FunctionList& dsts, const FunctionList& rhss, double relax, uint_t level, const Selection& flag, bool backwards ) const
   {
      const uint_t nf = dsts.size();
      if ( storage_->useBatchSor( level ) )
      {
         const auto    masks = batchMasks( nf, flag, HYTEG_HIP_MASK_ALL );
         const double* table = stencilTable( level, nf );
         forBatchChunks( nf, [&]( int first, int count ) {
            const auto u = batchPointers( dsts, level, first, count ), r = batchPointers( rhss, level, first, count );
            hipCheck( hyteg_hip_p1_sor_cells( count, u.data(), r.data(), (int) level, table + (size_t) first * 225, relax, backwards ? 1 : 0,
                                              masks.data() + first, storage_->stream() ),
                      "smooth_sor: cells (batched)" );
         } );
         return;
      }
      for ( uint_t k = 0; k < nf; ++k )
         storage_->forLocalCells( [&]( uint_t c, const MacroCell& cell ) {
            const unsigned mask = storage_->maskFor( cell, flag );
            if ( ( mask & HYTEG_HIP_MASK_INNER ) && level >= HYTEG_HIP_MIN_LEVEL )
               hipCheck( hyteg_hip_p1_sor_cell( dsts[k].get().getCellPointer( c, level ), rhss[k].get().getCellPointer( c, level ), (int) level,
                                                getCellStencils( cell.id, level ).inner, relax, backwards ? 1 : 0, storage_->stream() ),
                         "smooth_sor: cell" );
         } );
   }
   void launchSorShell( const FunctionList& dsts, const FunctionList& rhss, const FunctionList& rests, double relax, uint_t level, const Selection& flag,
                        unsigned bits, bool backwards ) const
   {
      const uint_t nf = dsts.size();
      if ( storage_->useBatchSor( level ) )
      {
         const auto                        masks = batchMasks( nf, flag, bits & HYTEG_HIP_MASK_SHELL );
         const hyteg_hip_sor_shell_tables* table = shellTable( level, nf );
         forBatchChunks( nf, [&]( int first, int count ) {
            const auto u = batchPointers( dsts, level, first, count ), r = batchPointers( rhss, level, first, count ),
                       q = batchPointers( rests, level, first, count );
            hipCheck( hyteg_hip_p1_sor_shell_cells( count, u.data(), r.data(), q.data(), (int) level, table + first, relax, masks.data() + first,
                                                    backwards ? 1 : 0, storage_->stream() ),
                      "smooth_sor: shell (batched)" );
         } );
         return;
      }
      for ( uint_t k = 0; k < nf; ++k )
         storage_->forLocalCells( [&]( uint_t c, const MacroCell& cell ) {
            const auto&    T    = sorTables_.at( level ).at( cell.id );
            const unsigned mask = storage_->maskFor( cell, flag ) & bits;
            hipCheck( hyteg_hip_p1_sor_shell_cell( dsts[k].get().getCellPointer( c, level ), rhss[k].get().getCellPointer( c, level ),
                                                   rests[k].get().getCellPointer( c, level ), (int) level, &T.edgeVerts[0][0], &T.edgeW[0][0],
                                                   &T.faceVerts[0][0], &T.faceW[0][0], T.vertexW, relax, mask, backwards ? 1 : 0,
                                                   storage_->stream() ),
                      "smooth_sor: shell" );
         } );
   }

 public:
   void smooth_gs( const P1Function< double >& dst, const P1Function< double >& rhs, uint_t level, const Selection& flag ) const
   {
      smooth_sor( dst, rhs, 1.0, level, flag, false );
   }
   void smooth_sor_backwards( const P1Function< double >& dst, const P1Function< double >& rhs, double relax, uint_t level, const Selection& flag ) const
   {
      smooth_sor( dst, rhs, relax, level, flag, true );
   }

   // P1Operator::computeInverseDiagonalOperatorValues, P1Operator.hpp:461-465, 636-906
   void computeInverseDiagonalOperatorValues()
   {
      inverseDiagonalValues_.reset( new P1Function< double >( "inverse diagonal entries", storage_, minLevel_, maxLevel_ ) );
      for ( uint_t l = minLevel_; l <= maxLevel_; ++l )
         for ( uint_t c = 0; c < storage_->getNumberOfLocalCells(); ++c )
         {
            const MacroCell& cell = storage_->getLocalCell( c );
            double*          d    = inverseDiagonalValues_->getCellPointer( c, l );
            hipCheck( hyteg_hip_p1_set_cell_masked( d, 1.0 / getCellStencils( cell.id, l ).inner[stencil::C], (int) l, HYTEG_HIP_MASK_INNER,
                                                    storage_->stream() ),
                      "inverse diagonal" );
            for ( int s = 0; s < 14; ++s )
            {
               // centre weight of a shared DoF = sum of the neighbour cells' shares (the reference adds the per-cell
               // centre entries of faceStencil3D / edgeStencil3D, P1Operator.hpp:700-870)
               const MacroPrimitive& p     = storage_->primitiveOfSlot( cell, s );
               double                total = 0.0;
               for ( int nc : p.cells )
               {
                  const MacroCell& other = storage_->getCells()[nc];
                  total += getCellStencils( nc, l ).slots[slotOf( other, p )][stencil::C];
               }
               hipCheck( hyteg_hip_p1_set_cell_masked( d, 1.0 / total, (int) l, 1u << s, storage_->stream() ), "inverse diagonal" );
            }
         }
   }
   std::shared_ptr< P1Function< double > > getInverseDiagonalValues() const
   {
      if ( !inverseDiagonalValues_ )
         throw std::runtime_error( "Inverse diagonal values have not been assembled, call computeInverseDiagonalOperatorValues() "
                                   "to set up this function." );
      return inverseDiagonalValues_;
   }

   // slot (0..13) under which primitive p appears in cell c
   static int slotOf( const MacroCell& c, const MacroPrimitive& p )
   {
      auto local = [&]( int g ) {
         for ( int q = 0; q < 4; ++q )
            if ( c.v[q] == g )
               return q;
         throw std::runtime_error( "slotOf: primitive is not part of the cell" );
      };
      if ( p.v.size() == 1 )
         return 10 + local( p.v[0] );
      if ( p.v.size() == 2 )
      {
         int a = local( p.v[0] ), b = local( p.v[1] );
         if ( a > b )
            std::swap( a, b );
         for ( int e = 0; e < 6; ++e )
            if ( kCellEdgeVerts[e][0] == a && kCellEdgeVerts[e][1] == b )
               return e;
      }
      int l[3] = { local( p.v[0] ), local( p.v[1] ), local( p.v[2] ) };
      std::sort( l, l + 3 );
      for ( int f = 0; f < 4; ++f )
         if ( kCellFaceVerts[f][0] == l[0] && kCellFaceVerts[f][1] == l[1] && kCellFaceVerts[f][2] == l[2] )
            return 6 + f;
      throw std::runtime_error( "slotOf: not found" );
   }

 private:
   // Operator::apply with one launch for all local cells: every selected point gets (this cell's share of) its stencil sum,
   // then the shares of the shared points are summed.  Add needs the summed shares in a temporary first.
   void applyBatched( const P1Function< double >& src, const P1Function< double >& dst, uint_t level, const Selection& flag, UpdateType updateType ) const
   {
      const bool sharedAdd = updateType == Add && hasSharedPoints( level, flag );
      auto       run       = [&]( const P1Function< double >& out, unsigned keep, int update ) {
         const auto masks = storage_->masksFor( flag, false, keep );
         storage_->forCellChunks( [&]( int first, int count ) {
            const auto d = out.cellPointers( level, first, count ), u = src.cellPointers( level, first, count );
            hipCheck( hyteg_hip_p1_apply_cells( count, d.data(), u.data(), (int) level, stencilTable( level ) + (size_t) first * 225,
                                                masks.data() + first, update, storage_->stream() ),
                      "apply (batched)" );
         } );
      };
      if ( !sharedAdd )
      {
         run( dst, HYTEG_HIP_MASK_ALL, hipUpdate( updateType ) );
         dst.sumSharedCopies( level, flag );
         return;
      }
      const auto tmp = P1Function< double >::zeroedScratch( "apply_tmp", storage_, level );
      run( dst, HYTEG_HIP_MASK_INNER, HYTEG_HIP_ADD );
      run( *tmp, HYTEG_HIP_MASK_SHELL, HYTEG_HIP_REPLACE );
      tmp->sumSharedCopies( level, flag );
      const auto masks = storage_->masksFor( flag, false, HYTEG_HIP_MASK_SHELL );
      storage_->forCellChunks( [&]( int first, int count ) {
         const auto   d = dst.cellPointers( level, first, count ), t = tmp->cellPointers( level, first, count );
         const double one = 1.0;
         hipCheck( hyteg_hip_p1_vector_cells( 1, count, d.data(), 1, t.data(), &one, (int) level, masks.data() + first, storage_->stream() ),
                   "apply: add shell (batched)" );
      } );
   }
 public:
   // ---- the whole CG solve in one launch for problems that fit one workgroup (hyteg_hip_p1_cg_small_cells) ----
   bool canCgSolveSmall( uint_t level ) const
   {
      const size_t n = storage_->getNumberOfLocalCells();
      return storage_->numRanks() == 1 && n >= 1 && n <= HYTEG_HIP_MAX_BATCH &&
             (int64_t) n * layout::cellSize( (int) level ) <= hyteg_hip_p1_cg_small_max_entries();
   }
   // the kernel takes the group lists of two exchange classes: with more taking part (three boundary parts that are all
   // selected) the solve goes through the multi-launch device CG
   bool cgSmallClassesFit( const P1Function< double >& x, uint_t level, const Selection& flagIn ) const
   {
      return sharedClasses( level, x.effectiveFlag( flagIn ) ).size() <= 2;
   }
   void cgSolveSmall( const P1Function< double >& x, const P1Function< double >& b, uint_t level, const Selection& flagIn, uint_t maxIter, double relTol,
                      double absTol, double* infoDev ) const
   {
      const Selection flag = x.effectiveFlag( flagIn ); // the function's boundary condition decides what `Inner` means
      const int  count = (int) storage_->getNumberOfLocalCells();
      const auto masks = storage_->masksFor( flag ), owned = storage_->masksFor( flag, true );
      const auto xs = x.cellPointers( level, 0, count ), bs = b.cellPointers( level, 0, count );
      const int* gp[2] = { nullptr, nullptr }, *ec[2] = { nullptr, nullptr }, *eo[2] = { nullptr, nullptr };
      int        ng[2] = { 0, 0 };
      // the kernel takes the group lists of two classes: the (at most two, cgSmallClassesFit) that take part, in ascending order
      const std::vector< int > classes = sharedClasses( level, flag );
      if ( classes.size() > 2 )
         throw std::runtime_error( "cgSolveSmall: more than two exchange classes take part (cgSmallClassesFit)" );
      int slot = 0;
      for ( int cls : classes )
      {
         const auto& plan = storage_->devicePlan( (int) level, cls );
         gp[slot] = plan.dGroupPtr, ec[slot] = plan.dEntryBuf, eo[slot] = plan.dEntryOff, ng[slot] = plan.ngroups();
         ++slot;
      }
      hipCheck( hyteg_hip_p1_cg_small_cells( count, xs.data(), bs.data(), (int) level, stencilTable( level ), masks.data(), owned.data(), gp, ec,
                                             eo, ng, (int) maxIter, relTol, absTol, infoDev, storage_->stream() ),
                "cgSolveSmall" );
   }

 private:
   // device tables of the batched kernels, one entry per local cell, the list repeated nf times (a batch of several functions is
   // ordered [function][cell]); built on first use, owned by the storage
   template < typename T, typename Build >
   const T* deviceTable( std::map< std::pair< uint_t, uint_t >, const T* >& cache, uint_t level, uint_t nf, Build&& hostTable ) const
   {
      const auto key = std::make_pair( level, nf );
      const auto it  = cache.find( key );
      if ( it != cache.end() )
         return it->second;
      const std::vector< T > once = hostTable();
      std::vector< T >       h;
      for ( uint_t k = 0; k < nf; ++k )
         h.insert( h.end(), once.begin(), once.end() );
      return cache[key] = static_cast< const T* >( storage_->uploadBytes( h.data(), h.size() * sizeof( T ) ) );
   }
   // [local cell][15 point classes][15 weights]: classes 0..13 the cell's shares, 14 inner
   const double* stencilTable( uint_t level, uint_t nf = 1 ) const
   {
      return deviceTable( stencilTables_, level, nf, [&] { return stencilTableHost( level ); } );
   }
   // the same shape with the weights of smooth_sor's `rest` (no inner class)
   const double* restTable( uint_t level, uint_t nf = 1 ) const
   {
      return deviceTable( restTables_, level, nf, [&] { return restTableHost( level ); } );
   }
   const hyteg_hip_sor_shell_tables* shellTable( uint_t level, uint_t nf = 1 ) const
   {
      return deviceTable( shellTables_, level, nf, [&] { return shellTableHost( level ); } );
   }
   std::vector< double > stencilTableHost( uint_t level ) const
   {
      std::vector< double > h;
      for ( int id : storage_->getLocalCellIDs() )
      {
         const auto& S = getCellStencils( id, level );
         h.insert( h.end(), &S.slots[0][0], &S.slots[0][0] + 14 * 15 );
         h.insert( h.end(), S.inner, S.inner + 15 );
      }
      return h;
   }
   std::vector< double > restTableHost( uint_t level ) const
   {
      std::vector< double > h;
      for ( int id : storage_->getLocalCellIDs() )
      {
         const auto& T = sorTables_.at( level ).at( id );
         h.insert( h.end(), &T.rest[0][0], &T.rest[0][0] + 14 * 15 );
         h.insert( h.end(), 15, 0.0 );
      }
      return h;
   }
   std::vector< hyteg_hip_sor_shell_tables > shellTableHost( uint_t level ) const
   {
      std::vector< hyteg_hip_sor_shell_tables > h;
      for ( int id : storage_->getLocalCellIDs() )
      {
         const auto&                T = sorTables_.at( level ).at( id );
         hyteg_hip_sor_shell_tables r{};
         std::memcpy( r.edge_verts, T.edgeVerts, sizeof( r.edge_verts ) );
         std::memcpy( r.face_verts, T.faceVerts, sizeof( r.face_verts ) );
         std::memcpy( r.edge_w, T.edgeW, sizeof( r.edge_w ) );
         std::memcpy( r.face_w, T.faceW, sizeof( r.face_w ) );
         std::memcpy( r.vertex_w, T.vertexW, sizeof( r.vertex_w ) );
         h.push_back( r );
      }
      return h;
   }
   // total weights and sweep orientations of every macro-primitive, handed to each adjacent cell in its local numbering
   std::vector< stencil::CellSorTables > buildSorTables( const std::vector< stencil::CellStencils >& S ) const
   {
      using namespace stencil;
      const auto&                   cells = storage_->getCells();
      std::vector< CellSorTables >  T( cells.size() );
      std::vector< std::array< double, 3 > > edgeTot( storage_->getEdges().size(), std::array< double, 3 >{} );
      std::vector< std::array< double, 7 > > faceTot( storage_->getFaces().size(), std::array< double, 7 >{} );
      std::vector< double >                  vertTot( storage_->getVertices().size(), 0.0 );
      for ( const auto& c : cells )
      {
         CellSorTables& t = T[c.id];
         for ( int s = 0; s < 14; ++s )
            for ( int k = 0; k < 15; ++k )
               t.rest[s][k] = k == C ? 0.0 : S[c.id].slots[s][k];
         for ( int k = 0; k < 4; ++k )
            vertTot[c.v[k]] += S[c.id].slots[10 + k][C];
         for ( int e = 0; e < 6; ++e )
         {
            int lo = kCellEdgeVerts[e][0], hi = kCellEdgeVerts[e][1];
            if ( c.v[lo] > c.v[hi] )
               std::swap( lo, hi );
            const int kp = offsetIndex( kUnit[hi][0] - kUnit[lo][0], kUnit[hi][1] - kUnit[lo][1], kUnit[hi][2] - kUnit[lo][2] );
            const int km = offsetIndex( kUnit[lo][0] - kUnit[hi][0], kUnit[lo][1] - kUnit[hi][1], kUnit[lo][2] - kUnit[hi][2] );
            t.edgeVerts[e][0] = lo, t.edgeVerts[e][1] = hi;
            auto& tot = edgeTot[c.edges[e]];
            tot[0] += S[c.id].slots[e][C], tot[1] += S[c.id].slots[e][km], tot[2] += S[c.id].slots[e][kp];
            t.rest[e][km] = t.rest[e][kp] = 0.0;
         }
         for ( int f = 0; f < 4; ++f )
         {
            int l[3] = { kCellFaceVerts[f][0], kCellFaceVerts[f][1], kCellFaceVerts[f][2] };
            std::sort( l, l + 3, [&]( int a, int b ) { return c.v[a] < c.v[b]; } );
            auto& tot = faceTot[c.faces[f]];
            tot[0] += S[c.id].slots[6 + f][C];
            for ( int d = 0; d < 6; ++d )
            {
               int o[3];
               for ( int r = 0; r < 3; ++r )
                  o[r] = kFaceDirs[d][0] * ( kUnit[l[1]][r] - kUnit[l[0]][r] ) + kFaceDirs[d][1] * ( kUnit[l[2]][r] - kUnit[l[0]][r] );
               const int k = offsetIndex( o[0], o[1], o[2] );
               tot[1 + d] += S[c.id].slots[6 + f][k];
               t.rest[6 + f][k] = 0.0;
            }
            for ( int r = 0; r < 3; ++r )
               t.faceVerts[f][r] = l[r];
         }
      }
      for ( const auto& c : cells )
      {
         CellSorTables& t = T[c.id];
         for ( int k = 0; k < 4; ++k )
            t.vertexW[k] = vertTot[c.v[k]];
         for ( int e = 0; e < 6; ++e )
            for ( int k = 0; k < 3; ++k )
               t.edgeW[e][k] = edgeTot[c.edges[e]][k];
         for ( int f = 0; f < 4; ++f )
            for ( int k = 0; k < 7; ++k )
               t.faceW[f][k] = faceTot[c.faces[f]][k];
      }
      return T;
   }
   // one rank, per-cell kernels and no shell point selected on any local cell: an apply (or residual) on these arguments consists
   // of the cells' interior launches and nothing else
   bool pureInterior( uint_t level, const Selection& flag ) const
   {
      return storage_->numRanks() == 1 && !storage_->useBatch( level ) && level >= HYTEG_HIP_MIN_LEVEL && !storage_->anyShellSelected( flag );
   }
   bool hasSharedPoints( uint_t level, const Selection& flag ) const
   {
      return !sharedClasses( level, flag ).empty();
   }
   // the exchange classes that take part under the selection and have shared points on this rank
   std::vector< int > sharedClasses( uint_t level, const Selection& flag ) const
   {
      std::vector< int > classes;
      for ( int cls = 0; cls < storage_->numClasses(); ++cls )
         if ( storage_->classSelected( cls, flag ) && storage_->exchangePlan( (int) level, cls ).ngroups() > 0 )
            classes.push_back( cls );
      return classes;
   }

   std::shared_ptr< PrimitiveStorage >                        storage_;
   uint_t                                                     minLevel_, maxLevel_;
   uint64_t                                                   uid_ = nextUid();
   std::map< uint_t, std::vector< stencil::CellStencils > >   stencils_;
   std::map< uint_t, std::vector< stencil::CellSorTables > >  sorTables_;
   mutable std::map< std::pair< uint_t, uint_t >, std::unique_ptr< P1Function< double > > > sorRest_; // (level, k): scratch of function k
   mutable std::map< std::pair< uint_t, uint_t >, const double* >                         stencilTables_, restTables_; // (level, nf)
   mutable std::map< std::pair< uint_t, uint_t >, const hyteg_hip_sor_shell_tables* >     shellTables_;
   std::shared_ptr< P1Function< double > >                    inverseDiagonalValues_;
};

using P1ConstantLaplaceOperator = P1ConstantOperator< forms::P1LaplaceForm >; // P1ConstantOperator.hpp:167-168
using P1ConstantMassOperator    = P1ConstantOperator< forms::P1MassForm >;

} // namespace hyteg
