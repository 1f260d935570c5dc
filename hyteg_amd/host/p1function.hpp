// p1function.hpp -- part of the C++ host layer above the C-ABI (see hyteg_host.hpp for the data model).
// P1Function< double > (= vertexdof::VertexDoFFunction< double >, src/hyteg/p1functionspace/VertexDoFFunction.cpp)
#pragma once

#include "storage.hpp"

namespace hyteg {

// =====================================================================================================
// P1Function< double > (= vertexdof::VertexDoFFunction< double >)
// =====================================================================================================
template < typename ValueType >
class P1Function
{
   static_assert( std::is_same< ValueType, double >::value,
                  "only double is supported, like the reference's generated 3D kernels (P1ConstantOperator.cpp:417-420)" );

 public:
   using valueType = ValueType;

   uint64_t uid() const { return uid_; }

   // BoundaryCondition::createAllInnerBC() (the pressure of P1StokesFunction, composites/P1StokesFunction.hpp:41-42): every
   // point of this function counts as Inner, whatever the storage says about the macro-primitive it lies on.  Default:
   // the storage's boundary types (create0123BC).  Operators, grid transfer and the function's own methods translate the
   // DoFType flag they are given with the destination function's boundary condition, as the reference does with
   // dst.getBoundaryCondition().getBoundaryType( primitive.getMeshBoundaryFlag() ) (P1Operator.hpp:301-303).
   // setBoundaryConditionAllInner( on ) is shorthand for setBoundaryCondition( createAllInnerBC() ) / the storage's default.
   void setBoundaryConditionAllInner( bool on = true )
   {
      bc_  = on ? std::make_shared< const BoundaryCondition >( BoundaryCondition::createAllInnerBC() ) : nullptr;
      uid_ = nextUid(); // a launch graph recorded with this function holds the masks of its former condition
   }
   bool hasAllInnerBoundaryCondition() const { return bc_ && bc_->allInner(); }
   // Function::setBoundaryCondition / getBoundaryCondition: the function's own map from mesh boundary flags to DoFTypes
   void setBoundaryCondition( const BoundaryCondition& bc )
   {
      bc_  = std::make_shared< const BoundaryCondition >( bc );
      uid_ = nextUid(); // as above
   }
   const BoundaryCondition& getBoundaryCondition() const { return bc_ ? *bc_ : storage_->getDefaultBoundaryCondition(); }
   // Function::copyBoundaryConditionFromFunction: what a temporary does with the function it stands in for
   template < typename OtherFunction >
   void copyBoundaryConditionFromFunction( const OtherFunction& other )
   {
      bc_ = other.boundaryConditionOrNull();
   }
   std::shared_ptr< const BoundaryCondition > boundaryConditionOrNull() const { return bc_; } // null: the storage's default
   // The one selection every mask of this function comes from.  Every method takes its flag as a Selection: a bare DoFType (or a
   // boundary of the condition, boundarySelection) is put under THIS function's condition here; one that an operator has already
   // put under its destination's condition passes unchanged, so that the temporaries it works with select the same points.
   Selection effectiveFlag( const Selection& s ) const { return s.resolved ? s : Selection( s.flag, bc_, s.uid, true ); }
   // the points of the primitives whose mesh flag belongs to one boundary of the function's condition
   Selection boundarySelection( const BoundaryUID& uid ) const
   {
      if ( !getBoundaryCondition().hasBoundary( uid ) )
         throw std::runtime_error( "P1Function '" + name_ + "': its boundary condition has no boundary '" + uid.name + "' with id " +
                                   std::to_string( uid.id ) + " (a BoundaryUID belongs to the condition that created it)" );
      return Selection( All, bc_, uid.id, true );
   }

   // scratch = true: arrays come from (and return to) the storage's scratch pool and are NOT zero-initialised
   P1Function( const std::string& name, const std::shared_ptr< PrimitiveStorage >& storage, uint_t minLevel, uint_t maxLevel,
               bool scratch = false )
   : name_( name )
   , storage_( storage )
   , minLevel_( minLevel )
   , maxLevel_( maxLevel )
   , scratch_( scratch )
   {
      if ( maxLevel > HYTEG_HIP_MAX_LEVEL || minLevel > maxLevel )
         throw std::runtime_error( "P1Function: bad level range" );
      storage->markInUse(); // the mesh boundary flags are fixed from here on
      const uint_t nLocal = storage->getNumberOfLocalCells();
      data_.resize( nLocal );
      for ( uint_t c = 0; c < nLocal; ++c )
         for ( uint_t l = minLevel; l <= maxLevel; ++l )
         {
            const size_t doubles = (size_t) layout::cellSize( (int) l );
            if ( scratch )
            {
               data_[c].push_back( storage->acquireScratch( doubles ) );
               continue;
            }
            void* p = nullptr;
            hipCheck( hyteg_hip_malloc( &p, doubles * sizeof( double ) ), "P1Function: malloc" );
            hipCheck( hyteg_hip_memset_zero( p, doubles * sizeof( double ), storage->stream() ), "P1Function: memset" );
            data_[c].push_back( static_cast< double* >( p ) );
         }
   }
   ~P1Function()
   {
      for ( auto& c : data_ )
         for ( uint_t l = 0; l < c.size(); ++l )
         {
            if ( scratch_ )
               storage_->releaseScratch( (size_t) layout::cellSize( (int) ( minLevel_ + l ) ), c[l] );
            else
               hyteg_hip_free( c[l] );
         }
   }
   P1Function( const P1Function& )            = delete;
   P1Function& operator=( const P1Function& ) = delete;

   const std::string&                  getFunctionName() const { return name_; }
   std::shared_ptr< PrimitiveStorage > getStorage() const { return storage_; }
   uint_t                              getMinLevel() const { return minLevel_; }
   uint_t                              getMaxLevel() const { return maxLevel_; }

   // device pointer of the array of local cell `c` at `level` (FunctionMemory::getPointer, FunctionMemory.hpp:109-113)
   double* getCellPointer( uint_t c, uint_t level ) const
   {
      checkLevel( level );
      return data_.at( c )[level - minLevel_];
   }

   // device pointers of local cells [first, first + count) at `level`
   std::vector< double* > cellPointers( uint_t level, int first, int count ) const
   {
      std::vector< double* > p;
      for ( int c = first; c < first + count; ++c )
         p.push_back( getCellPointer( (uint_t) c, level ) );
      return p;
   }

   // ---- interpolate ( VertexDoFFunction.cpp:380-392, :395-470 ) ----
   // Function::interpolate( constant | expr, level, BoundaryUID ): on the primitives whose mesh flag belongs to that boundary
   void interpolate( ValueType constant, uint_t level, const BoundaryUID& boundary ) const
   {
      interpolate( constant, level, boundarySelection( boundary ) );
   }
   void interpolate( const std::function< ValueType( const Point3D& ) >& expr, uint_t level, const BoundaryUID& boundary ) const
   {
      interpolate( expr, level, boundarySelection( boundary ) );
   }
   void interpolate( ValueType constant, uint_t level, const Selection& flagIn = All ) const
   {
      ScopedTimer timerFn( storage_->getTimingTree(), "P1Function" ), timerOp( storage_->getTimingTree(), "Interpolate" );
      const Selection flag = effectiveFlag( flagIn ); // the function's boundary condition decides what `Inner` means
      if ( storage_->useBatch( level ) )
      {
         const auto masks = storage_->masksFor( flag );
         storage_->forCellChunks( [&]( int first, int count ) {
            const auto dst = cellPointers( level, first, count );
            hipCheck( hyteg_hip_p1_vector_cells( 3, count, dst.data(), 0, nullptr, &constant, (int) level, masks.data() + first,
                                                 storage_->stream() ),
                      "interpolate (batched)" );
         } );
         return;
      }
      forCells( [&]( uint_t c, const MacroCell& cell ) {
         hipCheck( hyteg_hip_p1_set_cell_masked( getCellPointer( c, level ), constant, (int) level, storage_->maskFor( cell, flag ),
                                                 storage_->stream() ),
                   "interpolate" );
      } );
   }
   void interpolate( const std::function< ValueType( const Point3D& ) >& expr, uint_t level, const Selection& flagIn = All ) const
   {
      ScopedTimer timerFn( storage_->getTimingTree(), "P1Function" ), timerOp( storage_->getTimingTree(), "Interpolate" );
      const Selection flag = effectiveFlag( flagIn ); // the function's boundary condition decides what `Inner` means
      // evaluated on the host at the micro-vertex coordinates of VertexDoFMacroCell.hpp:70-77, then uploaded
      const int64_t N = layout::width( (int) level ), size = layout::cellSize( (int) level );
      P1Function    tmp( "interpolate_tmp", storage_, level, level, true );
      std::vector< double > host( (size_t) size );
      forCells( [&]( uint_t c, const MacroCell& cell ) {
         const double step = 1.0 / double( N - 1 );
         int64_t      k    = 0;
         for ( int64_t z = 0; z < N; ++z )
            for ( int64_t y = 0; y < N - z; ++y )
               for ( int64_t x = 0; x < N - z - y; ++x )
               {
                  Point3D p;
                  for ( int r = 0; r < 3; ++r )
                  {
                     const double xs = ( cell.coords[1][r] - cell.coords[0][r] ) * step;
                     const double ys = ( cell.coords[2][r] - cell.coords[0][r] ) * step;
                     const double zs = ( cell.coords[3][r] - cell.coords[0][r] ) * step;
                     p[r]            = cell.coords[0][r] + xs * double( x ) + ys * double( y ) + zs * double( z );
                  }
                  host[(size_t) k++] = expr( p );
               }
         hipCheck( hyteg_hip_upload( tmp.getCellPointer( c, level ), host.data(), (size_t) size * sizeof( double ), storage_->stream() ),
                   "interpolate: upload" );
         hipCheck( hyteg_hip_stream_synchronize( storage_->stream() ), "interpolate: sync" );
      } );
      // the copies of a shared DoF are evaluated from different cells' coordinates: make them bit-identical
      tmp.syncSharedCopies( level );
      assign( { 1.0 }, { tmp }, level, flag );
   }

   // ---- assign / add / multElementwise ( VertexDoFFunction.cpp:1130-1221, :1408-1484, :1487-1563 ) ----
   // `keep`: further restriction to point classes (HYTEG_HIP_MASK_INNER: inside the macro-cells, HYTEG_HIP_MASK_SHELL: on shared primitives)
   void assign( const std::vector< ValueType >&                                           scalars,
                const std::vector< std::reference_wrapper< const P1Function< ValueType > > >& functions,
                uint_t                                                                    level,
                const Selection&                                                          flag = All,
                unsigned                                                                  keep = HYTEG_HIP_MASK_ALL ) const
   {
      vectorOp( 0, scalars, functions, level, flag, keep );
   }
   void add( const std::vector< ValueType >&                                           scalars,
             const std::vector< std::reference_wrapper< const P1Function< ValueType > > >& functions,
             uint_t                                                                    level,
             const Selection&                                                          flag = All,
             unsigned                                                                  keep = HYTEG_HIP_MASK_ALL ) const
   {
      vectorOp( 1, scalars, functions, level, flag, keep );
   }
   void multElementwise( const std::vector< std::reference_wrapper< const P1Function< ValueType > > >& functions,
                         uint_t                                                                    level,
                         const Selection&                                                          flag = All,
                         unsigned                                                                  keep = HYTEG_HIP_MASK_ALL ) const
   {
      vectorOp( 2, {}, functions, level, flag, keep );
   }
   void setToZero( uint_t level ) const { interpolate( ValueType( 0 ), level, All ); }

   // ---- Operator::apply with UpdateType Add where cells share points: every cell's partial result of a shared DoF goes to a
   // zeroed scratch function, is summed over the cells there (sumSharedCopies) and the sum is added to the destination ----
   static std::unique_ptr< P1Function > zeroedScratch( const std::string& name, const std::shared_ptr< PrimitiveStorage >& storage, uint_t level )
   {
      std::unique_ptr< P1Function > f( new P1Function( name, storage, level, level, true ) );
      f->interpolate( ValueType( 0 ), level, All );
      return f;
   }
   // this += f on the macro-face, -edge and -vertex points `flag` selects, one launch per cell
   void addOnShell( const P1Function< ValueType >& f, uint_t level, const Selection& flagIn ) const
   {
      const Selection flag = effectiveFlag( flagIn );
      forCells( [&]( uint_t c, const MacroCell& cell ) {
         const double* srcs[1] = { f.getCellPointer( c, level ) };
         const double  one[1]  = { 1.0 };
         hipCheck( hyteg_hip_p1_vector_cell_masked( 1, getCellPointer( c, level ), 1, srcs, one, (int) level,
                                                    storage_->maskFor( cell, flag ) & HYTEG_HIP_MASK_SHELL, storage_->stream() ),
                   "addOnShell" );
      } );
   }

   // ---- dot ( VertexDoFFunction.cpp:1710-1793 ) ----
   ValueType dotLocal( const P1Function< ValueType >& rhs, uint_t level, const Selection& flagIn = All ) const
   {
      ScopedTimer timerFn( storage_->getTimingTree(), "P1Function" ), timerOp( storage_->getTimingTree(), "Dot (local)" );
      const Selection flag = effectiveFlag( flagIn ); // the function's boundary condition decides what `Inner` means
      // one result slot per local cell, a single download (= one host synchronisation) per dot product; the
      // workspace is reused cell after cell, which is safe because all launches are ordered on one stream
      const uint_t nLocal = storage_->getNumberOfLocalCells();
      if ( storage_->useBatch( level ) )
      {
         // one partial + one final launch per chunk of cells, one number per chunk comes back
         const auto masks  = storage_->masksFor( flag, true );
         int        nchunk = 0;
         storage_->forCellChunks( [&]( int first, int count ) {
            const auto a = cellPointers( level, first, count ), b = rhs.cellPointers( level, first, count );
            hipCheck( hyteg_hip_p1_dot_cells( count, a.data(), b.data(), (int) level, masks.data() + first, storage_->dotResult() + nchunk,
                                              storage_->dotWorkspace(), storage_->stream() ),
                      "dotLocal (batched)" );
            ++nchunk;
         } );
         std::vector< double > parts( (size_t) nchunk, 0.0 );
         hipCheck( hyteg_hip_download( parts.data(), storage_->dotResult(), parts.size() * sizeof( double ), storage_->stream() ),
                   "dotLocal: download" );
         double sum = 0.0;
         for ( double v : parts )
            sum += v;
         return sum;
      }
      forCells( [&]( uint_t c, const MacroCell& cell ) {
         hipCheck( hyteg_hip_p1_dot_cell_masked( getCellPointer( c, level ), rhs.getCellPointer( c, level ), (int) level,
                                                 storage_->ownedMaskFor( cell, flag ), storage_->dotResult() + c, storage_->dotWorkspace(),
                                                 storage_->stream() ),
                   "dotLocal" );
      } );
      std::vector< double > parts( nLocal, 0.0 );
      if ( nLocal > 0 )
         hipCheck( hyteg_hip_download( parts.data(), storage_->dotResult(), nLocal * sizeof( double ), storage_->stream() ),
                   "dotLocal: download" );
      double sum = 0.0;
      for ( double v : parts )
         sum += v; // cells in ascending order: deterministic
      return sum;
   }
   ValueType dotGlobal( const P1Function< ValueType >& rhs, uint_t level, const Selection& flag = All ) const
   {
      const double local = dotLocal( rhs, level, flag );
      ScopedTimer  timerFn( storage_->getTimingTree(), "P1Function" ), timerOp( storage_->getTimingTree(), "Dot (reduce)" );
      return storage_->allreduceSum( local, "dotGlobal" );
   }

   // ---- the vector body of a conjugate gradient iteration ( CGSolver.hpp:152-154 ) in one pass over the arrays:
   //      this->add( { alpha }, { p } );   r.add( { -alpha }, { ap } );   return r.dotGlobal( r )
   // One hyteg_hip_p1_cg_update_cells per chunk of cells (every copy of a shared DoF is updated, each DoF is counted once), one download,
   // one allreduce.  `this` and r carry the same boundary condition (CGSolver copies it).
   ValueType cgUpdate( const P1Function< ValueType >& r, const P1Function< ValueType >& p, const P1Function< ValueType >& ap, ValueType alpha,
                       uint_t level, const Selection& flagIn = All ) const
   {
      double local = 0.0;
      {
         ScopedTimer     timerFn( storage_->getTimingTree(), "P1Function" ), timerOp( storage_->getTimingTree(), "CG update" );
         const Selection flag        = effectiveFlag( flagIn ); // the function's boundary condition decides what `Inner` means
         const auto      updateMasks = storage_->masksFor( flag ), dotMasks = storage_->masksFor( flag, true );
         int             nchunk      = 0;
         storage_->forCellChunks( [&]( int first, int count ) {
            const auto xs = cellPointers( level, first, count ), rs = r.cellPointers( level, first, count );
            const auto ps = p.cellPointers( level, first, count ), aps = ap.cellPointers( level, first, count );
            hipCheck( hyteg_hip_p1_cg_update_cells( count, xs.data(), rs.data(), ps.data(), aps.data(), alpha, (int) level, updateMasks.data() + first,
                                                    dotMasks.data() + first, storage_->dotResult() + nchunk, storage_->dotWorkspace(),
                                                    storage_->stream() ),
                      "cgUpdate" );
            ++nchunk;
         } );
         std::vector< double > parts( (size_t) nchunk, 0.0 );
         if ( nchunk > 0 )
            hipCheck( hyteg_hip_download( parts.data(), storage_->dotResult(), parts.size() * sizeof( double ), storage_->stream() ),
                      "cgUpdate: download" );
         for ( double v : parts )
            local += v; // chunks in ascending order: deterministic
      }
      ScopedTimer timerFn( storage_->getTimingTree(), "P1Function" ), timerOp( storage_->getTimingTree(), "Dot (reduce)" );
      return storage_->allreduceSum( local, "cgUpdate" );
   }
   // ---- sum / max / min / max magnitude ( VertexDoFFunction.cpp:1796-1851, :1909-2057 ) ----
   // The statistics of this rank's DoFs, all from one pass over the arrays (hyteg_hip_p1_reduce_cells): one launch per chunk of
   // cells, one download, cells combined in ascending order.
   // Masks, as in the reference: the sums count every DoF once (owned masks) and the cell interiors only if `flag` contains Inner
   // (:1841-1847).  getMaxDoFValue, getMinDoFValue and getMaxDoFMagnitude do NOT flag-test the macro-cells (:1914-1918, :1964-1968,
   // :2014-2018): a cell's interior always takes part, whatever the flag, and only the faces, edges and vertices are selected by it.
   // That is the reference's behaviour and is kept.  With Inner in the flag the two sets of masks are the same and one pass serves
   // all five numbers; without it the extrema take a second pass under their own masks (still one download).
   struct Reduction
   {
      ValueType sum = 0, sumAbs = 0, min = std::numeric_limits< ValueType >::max(), max = -std::numeric_limits< ValueType >::max(),
                maxMagnitude = 0;
      // the other part of a composite function, or another cell, folded in
      void merge( const Reduction& o )
      {
         sum += o.sum, sumAbs += o.sumAbs;
         min = std::min( min, o.min ), max = std::max( max, o.max ), maxMagnitude = std::max( maxMagnitude, o.maxMagnitude );
      }
   };
   Reduction reduceLocal( uint_t level, const Selection& flagIn = All ) const
   {
      ScopedTimer timerFn( storage_->getTimingTree(), "P1Function" ), timerOp( storage_->getTimingTree(), "Sum (local)" );
      const Selection flag = effectiveFlag( flagIn ); // the function's boundary condition decides what `Inner` means
      return reduceArrays( *storage_, flag, [&]( int first, int count, const unsigned* masks, double* results ) {
         const auto a = cellPointers( level, first, count );
         hipCheck( hyteg_hip_p1_reduce_cells( count, a.data(), (int) level, masks, results, storage_->reduceWorkspace(), storage_->stream() ),
                   "reduceLocal" );
      } );
   }
   // shared with the edge-DoF part of P2Function: launch( first, count, masks, results_dev ) reduces a chunk of cells
   template < typename Launch >
   static Reduction reduceArrays( const PrimitiveStorage& storage, const Selection& flag, Launch&& launch )
   {
      const uint_t nLocal = storage.getNumberOfLocalCells();
      Reduction    r;
      if ( nLocal == 0 )
         return r;
      const auto              sumMasks = storage.masksFor( flag, true );
      std::vector< unsigned > extMasks = sumMasks;
      for ( unsigned& m : extMasks )
         m |= HYTEG_HIP_MASK_INNER;
      const uint_t sets = extMasks == sumMasks ? 1 : 2;
      double*      dev  = storage.reduceResult();
      storage.forCellChunks( [&]( int first, int count ) {
         launch( first, count, sumMasks.data() + first, dev + (size_t) first * HYTEG_HIP_REDUCE_COUNT );
         if ( sets == 2 )
            launch( first, count, extMasks.data() + first, dev + ( nLocal + (size_t) first ) * HYTEG_HIP_REDUCE_COUNT );
      } );
      std::vector< double > host( sets * nLocal * HYTEG_HIP_REDUCE_COUNT );
      hipCheck( hyteg_hip_download( host.data(), dev, host.size() * sizeof( double ), storage.stream() ), "reduceLocal: download" );
      for ( uint_t c = 0; c < nLocal; ++c ) // cells in ascending order: deterministic
      {
         const double* s = host.data() + c * HYTEG_HIP_REDUCE_COUNT;
         const double* e = host.data() + ( ( sets - 1 ) * nLocal + c ) * HYTEG_HIP_REDUCE_COUNT;
         r.sum += s[HYTEG_HIP_REDUCE_SUM], r.sumAbs += s[HYTEG_HIP_REDUCE_SUM_ABS];
         r.min          = std::min( r.min, e[HYTEG_HIP_REDUCE_MIN] );
         r.max          = std::max( r.max, e[HYTEG_HIP_REDUCE_MAX] );
         r.maxMagnitude = std::max( r.maxMagnitude, e[HYTEG_HIP_REDUCE_MAX_ABS] );
      }
      return r;
   }
   ValueType sumLocal( uint_t level, const Selection& flag = All, bool absolute = false ) const
   {
      const Reduction r = reduceLocal( level, flag );
      return absolute ? r.sumAbs : r.sum;
   }
   ValueType sumGlobal( uint_t level, const Selection& flag = All, bool absolute = false ) const
   {
      const double local = sumLocal( level, flag, absolute );
      ScopedTimer  timerFn( storage_->getTimingTree(), "P1Function" ), timerOp( storage_->getTimingTree(), "Sum (reduce)" );
      return storage_->allreduceSum( local, "sumGlobal" );
   }
   ValueType getMaxDoFValue( uint_t level, const Selection& flag = All, bool mpiReduce = true ) const
   {
      const double local = reduceLocal( level, flag ).max;
      return mpiReduce ? storage_->allreduceMax( local, "getMaxDoFValue" ) : local;
   }
   ValueType getMinDoFValue( uint_t level, const Selection& flag = All, bool mpiReduce = true ) const
   {
      const double local = reduceLocal( level, flag ).min;
      return mpiReduce ? -storage_->allreduceMax( -local, "getMinDoFValue" ) : local; // as at VertexDoFFunction.cpp:2053
   }
   ValueType getMaxDoFMagnitude( uint_t level, const Selection& flag = All, bool mpiReduce = true ) const
   {
      const double local = reduceLocal( level, flag ).maxMagnitude;
      return mpiReduce ? storage_->allreduceMax( local, "getMaxDoFMagnitude" ) : local;
   }
   // numberOfLocalDoFs / numberOfGlobalDoFs< P1FunctionTag > (src/hyteg/functions/FunctionTools.hpp): what the sum of ones gives
   uint64_t numberOfLocalDoFs( uint_t level ) const { return storage_->numberOfDoFs( level, 0, false ); }
   uint64_t numberOfGlobalDoFs( uint_t level ) const { return storage_->numberOfDoFs( level, 0, true ); }

   // ---- shared-point exchange (the cell-centric replacement of communicate<> / communicateAdditively<>) ----
   // additive: every copy of a shared DoF := sum of all copies (VertexDoFAdditivePackInfo.hpp:676-745 + copy back)
   void sumSharedCopies( uint_t level, const Selection& flag = All ) const
   {
      exchangeBegin( level, flag );
      exchangeEnd( level, flag, true );
   }
   // every copy := the copy held by the lowest-numbered neighbour cell
   void syncSharedCopies( uint_t level, const Selection& flag = All ) const
   {
      exchangeBegin( level, flag );
      exchangeEnd( level, flag, false );
   }
   // split form: pack + start the transfer / wait + reduce.  Kernels that do not touch shared points may be
   // launched in between (the interior apply overlaps the halo exchange).
   void beginSumSharedCopies( uint_t level, const Selection& flag = All ) const { exchangeBegin( level, flag ); }
   void endSumSharedCopies( uint_t level, const Selection& flag = All ) const { exchangeEnd( level, flag, true ); }
   // beginSumSharedCopies for a caller whose boundary-share kernel delivers the shares itself
   // (PrimitiveStorage::sharedExchangeBeginByShares); flag: effective flag
   bool beginSumSharedCopiesByShares( uint_t level, const Selection& flag, PrimitiveStorage::ShareSend& out ) const
   {
      checkLevel( level );
      return storage_->sharedExchangeBeginByShares( (int) level, flag, out );
   }

   void copyCellToHost( uint_t c, uint_t level, double* host ) const
   {
      hipCheck( hyteg_hip_download( host, getCellPointer( c, level ), (size_t) layout::cellSize( (int) level ) * sizeof( double ),
                                    storage_->stream() ),
                "copyCellToHost" );
      // the host is about to use values that may have come through a peer-to-peer exchange: a timed-out arrival wait fails here
      storage_->checkTransportAtHostRead();
   }
   void copyCellFromHost( uint_t c, uint_t level, const double* host ) const
   {
      hipCheck( hyteg_hip_upload( getCellPointer( c, level ), host, (size_t) layout::cellSize( (int) level ) * sizeof( double ),
                                  storage_->stream() ),
                "copyCellFromHost" );
      hipCheck( hyteg_hip_stream_synchronize( storage_->stream() ), "copyCellFromHost: sync" );
   }

 private:
   void checkLevel( uint_t level ) const
   {
      if ( level < minLevel_ || level > maxLevel_ )
         throw std::runtime_error( "P1Function '" + name_ + "': level " + std::to_string( level ) + " not allocated" );
   }
   template < typename F >
   void forCells( F&& fn ) const
   {
      for ( uint_t c = 0; c < storage_->getNumberOfLocalCells(); ++c )
         fn( c, storage_->getLocalCell( c ) );
   }
   void vectorOp( int                                                                       op,
                  const std::vector< ValueType >&                                           scalars,
                  const std::vector< std::reference_wrapper< const P1Function< ValueType > > >& functions,
                  uint_t                                                                    level,
                  const Selection&                                                          flagIn,
                  unsigned                                                                  keep = HYTEG_HIP_MASK_ALL ) const
   {
      const Selection flag = effectiveFlag( flagIn ); // the function's boundary condition decides what `Inner` means
      static const char* kOpNames[3] = { "Assign", "Add", "Multiply elementwise" };
      ScopedTimer        timerFn( storage_->getTimingTree(), "P1Function" ), timerOp( storage_->getTimingTree(), kOpNames[op] );
      if ( functions.empty() || functions.size() > HYTEG_HIP_MAX_SRCS || ( op != 2 && scalars.size() != functions.size() ) )
         throw std::runtime_error( "P1Function::assign/add/multElementwise: bad number of functions or scalars" );
      if ( storage_->useBatch( level ) )
      {
         const auto masks = storage_->masksFor( flag, false, keep );
         storage_->forCellChunks( [&]( int first, int count ) {
            const auto             dst = cellPointers( level, first, count );
            std::vector< double* > srcs; // [function][cell]
            for ( const auto& f : functions )
               for ( double* q : f.get().cellPointers( level, first, count ) )
                  srcs.push_back( q );
            hipCheck( hyteg_hip_p1_vector_cells( op, count, dst.data(), (int) functions.size(), srcs.data(),
                                                 op == 2 ? nullptr : scalars.data(), (int) level, masks.data() + first, storage_->stream() ),
                      "P1Function vector op (batched)" );
         } );
         return;
      }
      forCells( [&]( uint_t c, const MacroCell& cell ) {
         const double* srcs[HYTEG_HIP_MAX_SRCS];
         for ( uint_t k = 0; k < functions.size(); ++k )
            srcs[k] = functions[k].get().getCellPointer( c, level );
         hipCheck( hyteg_hip_p1_vector_cell_masked( op, getCellPointer( c, level ), (int) functions.size(), srcs,
                                                    op == 2 ? nullptr : scalars.data(), (int) level, storage_->maskFor( cell, flag ) & keep,
                                                    storage_->stream() ),
                   "P1Function vector op" );
      } );
   }

 public:
   // assign (op 0) / add (op 1) with coefficients read from device memory when the kernels run; storages of one rank
   // with at most HYTEG_HIP_MAX_BATCH local cells (one launch)
   void vectorOpDeviceScalars( int op, const std::vector< const double* >& scalarPtrs,
                               const std::vector< std::reference_wrapper< const P1Function< ValueType > > >& functions, uint_t level,
                               const Selection& flagIn ) const
   {
      const Selection flag = effectiveFlag( flagIn ); // the function's boundary condition decides what `Inner` means
      const int  count = (int) storage_->getNumberOfLocalCells();
      const auto masks = storage_->masksFor( flag );
      const auto dst   = cellPointers( level, 0, count );
      std::vector< double* > srcs;
      for ( const auto& f : functions )
         for ( double* q : f.get().cellPointers( level, 0, count ) )
            srcs.push_back( q );
      hipCheck( hyteg_hip_p1_vector_cells_dev( op, count, dst.data(), (int) functions.size(), srcs.data(), scalarPtrs.data(), (int) level,
                                               masks.data(), storage_->stream() ),
                "P1Function vector op (device scalars)" );
   }
   // cgScalars[slot] = <this, rhs> over the points `flag` selects (each shared point counted once), then phase `phase` of
   // the conjugate gradient recurrences (hyteg_hip_cg_scalars), in one launch; no host synchronisation
   void dotLocalToCgScalars( const P1Function< ValueType >& rhs, uint_t level, const Selection& flagIn, double* cgScalars, int slot, int phase,
                             double relTol, double absTol ) const
   {
      const Selection flag = effectiveFlag( flagIn ); // the function's boundary condition decides what `Inner` means
      const int  count = (int) storage_->getNumberOfLocalCells();
      const auto masks = storage_->masksFor( flag, true );
      const auto a = cellPointers( level, 0, count ), b = rhs.cellPointers( level, 0, count );
      hipCheck( hyteg_hip_p1_dot_cells_cg( count, a.data(), b.data(), (int) level, masks.data(), cgScalars, slot, phase, relTol, absTol,
                                           storage_->dotWorkspace(), storage_->stream() ),
                "dotLocalToCgScalars" );
   }

 private:
   std::vector< double* > cellArrays( uint_t level ) const
   {
      std::vector< double* > a;
      for ( uint_t c = 0; c < storage_->getNumberOfLocalCells(); ++c )
         a.push_back( getCellPointer( c, level ) );
      return a;
   }
   void exchangeBegin( uint_t level, const Selection& flagIn ) const
   {
      const Selection flag = effectiveFlag( flagIn ); // the function's boundary condition decides what `Inner` means
      checkLevel( level );
      storage_->sharedExchangeBegin( cellArrays( level ), (int) level, flag, 0 );
   }
   void exchangeEnd( uint_t level, const Selection& flagIn, bool additive ) const
   {
      const Selection flag = effectiveFlag( flagIn ); // the function's boundary condition decides what `Inner` means
      storage_->sharedExchangeEnd( cellArrays( level ), (int) level, flag, 0, additive );
   }

   std::string                                                           name_;
   std::shared_ptr< PrimitiveStorage >                                   storage_;
   uint_t                                                                minLevel_, maxLevel_;
   bool                                                                  scratch_ = false;
   std::shared_ptr< const BoundaryCondition >                            bc_; // null: the storage's default condition
   uint64_t                                                              uid_     = nextUid();
   std::vector< std::vector< double* > >                                 data_;
};

// ---- what the elementwise operators share (p1elementwise.hpp, p1divkgrad.hpp, p1epsilon.hpp) ----

// a macro-cell's vertices as the macro_vertex_coords of the C-ABI
inline void coordsOf( const MacroCell& cell, double cc[12] )
{
   for ( int v = 0; v < 4; ++v )
      for ( int r = 0; r < 3; ++r )
         cc[3 * v + r] = cell.coords[v][r];
}

// P1Function::invertElementwise of an assembled diagonal: set-up time, on the host
inline void invertElementwise( const P1Function< double >& f, uint_t level )
{
   std::vector< double > h( (size_t) hyteg_hip_cell_size( (int) level ) );
   f.getStorage()->forLocalCells( [&]( uint_t c, const MacroCell& ) {
      f.copyCellToHost( c, level, h.data() );
      for ( double& v : h )
         v = v != 0.0 ? 1.0 / v : 0.0;
      f.copyCellFromHost( c, level, h.data() );
   } );
}

// the three vector passes of P1ElementwiseOperator::smooth_jac that follow dst = A src (P1ElementwiseOperator.cpp:288-331),
//   dst = rhs - dst ; dst = invDiag .* dst ; dst = src + omega dst,   on the shell classes `shell` of cell c
inline void smoothJacShellPasses( const P1Function< double >& dst, const P1Function< double >& rhs, const P1Function< double >& invDiag,
                                  const P1Function< double >& src, double omega, uint_t c, uint_t level, unsigned shell )
{
   if ( !shell )
      return;
   const hyteg_hip_stream_t stream = dst.getStorage()->stream();
   double*                  d      = dst.getCellPointer( c, level );
   const double*            a[2]   = { rhs.getCellPointer( c, level ), d };
   const double             s1[2]  = { 1.0, -1.0 };
   hipCheck( hyteg_hip_p1_vector_cell_masked( 0, d, 2, a, s1, (int) level, shell, stream ), "smooth_jac: shell residual" );
   const double* m[2] = { invDiag.getCellPointer( c, level ), d };
   hipCheck( hyteg_hip_p1_vector_cell_masked( 2, d, 2, m, nullptr, (int) level, shell, stream ), "smooth_jac: shell scale" );
   const double* u[2]  = { src.getCellPointer( c, level ), d };
   const double  s2[2] = { 1.0, omega };
   hipCheck( hyteg_hip_p1_vector_cell_masked( 0, d, 2, u, s2, (int) level, shell, stream ), "smooth_jac: shell update" );
}

// the vector passes of a residual or of a Chebyshev step that follow t = A src (GeometricMultigridSolver.hpp:240-246,
// ChebyshevSmoother.hpp:165-212), each where its function is given,
//   t = rhs - t ; t = invDiag .* t ; x = x + c t,   on the shell classes `shell` of cell ci
inline void fusedStepShellPasses( const P1Function< double >& t, const P1Function< double >* rhs, const P1Function< double >* invDiag,
                                  const P1Function< double >* x, double c, uint_t ci, uint_t level, unsigned shell )
{
   if ( !shell )
      return;
   const hyteg_hip_stream_t stream = t.getStorage()->stream();
   double*                  d      = t.getCellPointer( ci, level );
   if ( rhs )
   {
      const double* a[2]  = { rhs->getCellPointer( ci, level ), d };
      const double  s1[2] = { 1.0, -1.0 };
      hipCheck( hyteg_hip_p1_vector_cell_masked( 0, d, 2, a, s1, (int) level, shell, stream ), "fused step: shell residual" );
   }
   if ( invDiag )
   {
      const double* m[2] = { invDiag->getCellPointer( ci, level ), d };
      hipCheck( hyteg_hip_p1_vector_cell_masked( 2, d, 2, m, nullptr, (int) level, shell, stream ), "fused step: shell scale" );
   }
   if ( x )
   {
      double*       xd    = x->getCellPointer( ci, level );
      const double* u[2]  = { xd, d };
      const double  s2[2] = { 1.0, c };
      hipCheck( hyteg_hip_p1_vector_cell_masked( 0, xd, 2, u, s2, (int) level, shell, stream ), "fused step: shell update" );
   }
}

// x += c t on the inner points of cell ci: closes a Chebyshev smoother call of order 1 (no step follows the start)
inline void chebyshevFinishCell( const P1Function< double >& x, const P1Function< double >& t, double c, uint_t ci, uint_t level, unsigned inner )
{
   if ( !inner || level < HYTEG_HIP_MIN_LEVEL )
      return;
   double*       d     = x.getCellPointer( ci, level );
   const double* u[2]  = { d, t.getCellPointer( ci, level ) };
   const double  sc[2] = { 1.0, c };
   hipCheck( hyteg_hip_p1_vector_cell_masked( 0, d, 2, u, sc, (int) level, inner, x.getStorage()->stream() ), "chebyshevFinish" );
}

} // namespace hyteg
