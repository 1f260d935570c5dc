// projectnormal.hpp -- part of the C++ host layer above the C-ABI (see hyteg_host.hpp for the data model).
// The strong free-slip boundary condition:
//   P1ProjectNormalOperator   src/hyteg/p1functionspace/P1ProjectNormalOperator.{hpp,cpp}, freeslip/VertexDoFProjectNormal.hpp
//   P2ProjectNormalOperator   src/hyteg/p2functionspace/P2ProjectNormalOperator.cpp:34-42, edgedofspace/freeslip/EdgeDoFProjectNormal.hpp
//   StrongFreeSlipWrapper     src/hyteg/composites/StrongFreeSlipWrapper.hpp:59-98
// The reference calls the normal function at every boundary point of every project(); here the constructor evaluates it once
// per level into one device table per macro-cell, [3][shell size] in the order of the shell enumeration
// (hyteg_hip_p1_shell_enumeration), and project() is one launch per chunk of cells (hyteg_hip_p1_project_normal_cells).
#pragma once

#include "stokes.hpp"
#include "taylorhood.hpp"

namespace hyteg {

namespace freeslip {

// Coordinates of a point of a macro-vertex, -edge or -face from the vertices of THAT PRIMITIVE (sorted global ids), not from the
// cell that looks at it: the copies of a shared point in different cells and on different ranks then get the same bits, and so
// do the normals evaluated there.  weight[k]: barycentric coordinate of the point with respect to cell vertex k, in units of
// `step` (integers for vertex DoFs, halves for the midpoints of micro-edges).
inline Point3D primitivePoint( const PrimitiveStorage& storage, const MacroCell& cell, const MacroPrimitive& prim, const double weight[4], double step )
{
   const Point3D& origin = storage.getVertexCoordinates( (uint_t) prim.v[0] );
   Point3D        p      = origin;
   for ( size_t m = 1; m < prim.v.size(); ++m )
   {
      int k = 0;
      while ( cell.v[(size_t) k] != prim.v[m] )
         ++k;
      const Point3D& vm = storage.getVertexCoordinates( (uint_t) prim.v[m] );
      for ( int r = 0; r < 3; ++r )
         p[r] += ( vm[r] - origin[r] ) * step * weight[k];
   }
   return p;
}

// x, y, z, slot per q of the kernels' shell enumeration (slot -1: q is skipped)
inline std::vector< std::array< int, 4 > > shellEnumeration( uint_t level )
{
   std::vector< std::array< int, 4 > > e( (size_t) hyteg_hip_p1_shell_size( (int) level ) );
   static_assert( sizeof( std::array< int, 4 > ) == 4 * sizeof( int ), "packed" );
   hipCheck( hyteg_hip_p1_shell_enumeration( (int) level, e.empty() ? nullptr : e[0].data() ), "shell enumeration" );
   return e;
}

// The points the normal function of a P1ProjectNormalOperator is evaluated at, in q order: the vertex DoFs on the primitives of
// the cell that lie on the domain boundary (faces with one neighbour cell, and the edges and vertices of such faces).  NaN
// everywhere else: the normal function may be singular inside the domain.  Host only.
inline std::vector< Point3D > shellPoints( const PrimitiveStorage& storage, const MacroCell& cell, uint_t level )
{
   const double           nan = std::numeric_limits< double >::quiet_NaN();
   const auto             e   = shellEnumeration( level );
   const int              n   = (int) layout::width( (int) level ) - 1;
   const double           step = n > 0 ? 1.0 / double( n ) : 0.0;
   std::vector< Point3D > pts( e.size(), Point3D{ nan, nan, nan } );
   for ( size_t q = 0; q < e.size(); ++q )
   {
      const int slot = e[q][3];
      if ( slot < 0 )
         continue;
      const MacroPrimitive& prim = storage.primitiveOfSlot( cell, slot );
      if ( !prim.onBoundary )
         continue;
      const double weight[4] = { double( n - e[q][0] - e[q][1] - e[q][2] ), double( e[q][0] ), double( e[q][1] ), double( e[q][2] ) };
      pts[q]                 = primitivePoint( storage, cell, prim, weight, step );
   }
   return pts;
}

// x, y, z, orientation, slot per q of the kernel's shell edge-DoF enumeration (slot -1: q is skipped)
inline std::vector< std::array< int, 5 > > edgeShellEnumeration( uint_t level )
{
   std::vector< std::array< int, 5 > > e( (size_t) hyteg_hip_p2_edge_shell_size( (int) level ) );
   hipCheck( hyteg_hip_p2_edge_shell_enumeration( (int) level, e.empty() ? nullptr : e[0].data() ), "shell edge enumeration" );
   return e;
}

// shellPoints for the edge DoFs: the midpoints of the micro-edges (EdgeDoFProjectNormal.hpp:112-124, 283-288) on the boundary
// primitives of the cell, in the order of the shell edge-DoF enumeration
inline std::vector< Point3D > edgeShellPoints( const PrimitiveStorage& storage, const MacroCell& cell, uint_t level )
{
   static const int       ends[6][2][3] = { { { 0, 0, 0 }, { 1, 0, 0 } }, { { 0, 0, 0 }, { 0, 1, 0 } }, { { 0, 0, 0 }, { 0, 0, 1 } },
                                            { { 1, 0, 0 }, { 0, 1, 0 } }, { { 1, 0, 0 }, { 0, 0, 1 } }, { { 0, 1, 0 }, { 0, 0, 1 } } };
   const double           nan  = std::numeric_limits< double >::quiet_NaN();
   const auto             e    = edgeShellEnumeration( level );
   const int              n    = 1 << level;
   const double           half = 0.5 / double( n ); // weights in units of half a micro-edge
   std::vector< Point3D > pts( e.size(), Point3D{ nan, nan, nan } );
   for ( size_t q = 0; q < e.size(); ++q )
   {
      const int slot = e[q][4];
      if ( slot < 0 )
         continue;
      const MacroPrimitive& prim = storage.primitiveOfSlot( cell, slot );
      if ( !prim.onBoundary )
         continue;
      const int* a = ends[e[q][3]][0];
      const int* b = ends[e[q][3]][1];
      const int  x2 = 2 * e[q][0] + a[0] + b[0], y2 = 2 * e[q][1] + a[1] + b[1], z2 = 2 * e[q][2] + a[2] + b[2];
      const double weight[4] = { double( 2 * n - x2 - y2 - z2 ), double( x2 ), double( y2 ), double( z2 ) };
      pts[q]                 = primitivePoint( storage, cell, prim, weight, half );
   }
   return pts;
}

// the selection must not take a primitive without normals: a face between two cells (VertexDoFProjectNormal.hpp:51-54), or an
// edge or vertex that is not part of a boundary face
inline void checkSelectedPrimitives( const PrimitiveStorage& storage, const Selection& sel )
{
   storage.forLocalCells( [&]( uint_t, const MacroCell& cell ) {
      const unsigned mask = storage.maskFor( cell, sel ) & HYTEG_HIP_MASK_SHELL;
      for ( int s = 0; s < 14; ++s )
      {
         if ( !( ( mask >> s ) & 1u ) || storage.primitiveOfSlot( cell, s ).onBoundary )
            continue;
         if ( s >= 6 && s < 10 )
            throw std::runtime_error( "Cannot project normals if not a boundary face" );
         throw std::runtime_error( "Cannot project normals at a macro-edge or macro-vertex inside the domain" );
      }
   } );
}

// device tables [local cell] of [3][entries] doubles, owned
class NormalTables
{
 public:
   NormalTables() = default;
   ~NormalTables()
   {
      for ( double* p : dev_ )
         hyteg_hip_free( p );
   }
   NormalTables( const NormalTables& )            = delete;
   NormalTables& operator=( const NormalTables& ) = delete;
   NormalTables( NormalTables&& o ) noexcept
   : dev_( std::move( o.dev_ ) )
   {
      o.dev_.clear();
   }
   // evaluates normal_function at the points that are not NaN; zero elsewhere
   void add( const PrimitiveStorage& storage, const std::vector< Point3D >& pts, const std::function< void( const Point3D&, Point3D& ) >& normal_function )
   {
      const size_t          S = pts.size();
      std::vector< double > h( 3 * std::max< size_t >( S, 1 ), 0.0 );
      for ( size_t q = 0; q < S; ++q )
      {
         if ( std::isnan( pts[q][0] ) )
            continue;
         Point3D n{ 0.0, 0.0, 0.0 };
         normal_function( pts[q], n );
         for ( size_t r = 0; r < 3; ++r )
            h[r * S + q] = n[r];
      }
      void* p = nullptr;
      hipCheck( hyteg_hip_malloc( &p, h.size() * sizeof( double ) ), "ProjectNormalOperator: malloc" );
      dev_.push_back( static_cast< double* >( p ) );
      hipCheck( hyteg_hip_upload( p, h.data(), h.size() * sizeof( double ), storage.stream() ), "ProjectNormalOperator: upload" );
      hipCheck( hyteg_hip_stream_synchronize( storage.stream() ), "ProjectNormalOperator: sync" );
   }
   const double* const* data() const { return dev_.data(); }

 private:
   std::vector< double* > dev_;
};

} // namespace freeslip

// P1ProjectNormalOperator.hpp: projects a velocity onto the tangential plane, ( I - n n^T ) ( u, v, w ), at the vertex DoFs of the
// primitives `flag` selects under the boundary condition of u.  n = normal_function( x ) is not normalised.
class P1ProjectNormalOperator
{
 public:
   P1ProjectNormalOperator( const std::shared_ptr< PrimitiveStorage >& storage, uint_t minLevel, uint_t maxLevel,
                            const std::function< void( const Point3D&, Point3D& ) >& normal_function )
   : storage_( storage )
   , minLevel_( minLevel )
   , maxLevel_( maxLevel )
   {
      if ( maxLevel > HYTEG_HIP_MAX_LEVEL || minLevel > maxLevel )
         throw std::runtime_error( "P1ProjectNormalOperator: bad level range" );
      storage->markInUse(); // the tables depend on which primitives are on the boundary
      for ( uint_t l = minLevel; l <= maxLevel; ++l )
      {
         tables_.emplace_back();
         storage->forLocalCells(
             [&]( uint_t, const MacroCell& cell ) { tables_.back().add( *storage, freeslip::shellPoints( *storage, cell, l ), normal_function ); } );
      }
   }

   // P1ProjectNormalOperator.cpp:39-120.  No allocation, no upload, no synchronisation: may be recorded into a launch graph.
   void project( const P1Function< double >& u, const P1Function< double >& v, const P1Function< double >& w, uint_t level, DoFType flag ) const
   {
      ScopedTimer timer( storage_->getTimingTree(), "Project" );
      if ( level < minLevel_ || level > maxLevel_ )
         throw std::runtime_error( "P1ProjectNormalOperator: level " + std::to_string( level ) + " not allocated" );
      // the per-primitive test of P1ProjectNormalOperator.cpp:53, 82, 106: the boundary condition of u decides
      const Selection sel = u.effectiveFlag( flag );
      freeslip::checkSelectedPrimitives( *storage_, sel );
      const auto masks = storage_->masksFor( sel, false, HYTEG_HIP_MASK_SHELL );
      storage_->forCellChunks( [&]( int first, int count ) {
         const auto us = u.cellPointers( level, first, count ), vs = v.cellPointers( level, first, count ), ws = w.cellPointers( level, first, count );
         hipCheck( hyteg_hip_p1_project_normal_cells( count, us.data(), vs.data(), ws.data(), tables_[level - minLevel_].data() + first, (int) level,
                                                      masks.data() + first, storage_->stream() ),
                   "P1ProjectNormalOperator::project" );
      } );
   }
   void project( const P1VectorFunction< double >& dst, uint_t level, DoFType flag ) const { project( dst[0], dst[1], dst[2], level, flag ); }
   void project( const P1StokesFunction< double >& dst, uint_t level, DoFType flag ) const { project( dst.uvw(), level, flag ); }

   std::shared_ptr< PrimitiveStorage > getStorage() const { return storage_; }
   uint_t                              getMinLevel() const { return minLevel_; }
   uint_t                              getMaxLevel() const { return maxLevel_; }

 private:
   std::shared_ptr< PrimitiveStorage >   storage_;
   uint_t                                minLevel_, maxLevel_;
   std::vector< freeslip::NormalTables > tables_; // [level - minLevel]
};

// P2ProjectNormalOperator.cpp:34-42: the vertex projection on the vertex-DoF parts plus the same projection on the edge-DoF parts,
// whose normals are evaluated at the midpoints of the micro-edges
class P2ProjectNormalOperator
{
 public:
   P2ProjectNormalOperator( const std::shared_ptr< PrimitiveStorage >& storage, uint_t minLevel, uint_t maxLevel,
                            const std::function< void( const Point3D&, Point3D& ) >& normal_function )
   : p1Operator_( storage, minLevel, maxLevel, normal_function )
   , storage_( storage )
   , minLevel_( minLevel )
   , maxLevel_( maxLevel )
   {
      if ( maxLevel > HYTEG_HIP_P2_MAX_LEVEL )
         throw std::runtime_error( "P2ProjectNormalOperator: bad level range" );
      for ( uint_t l = minLevel; l <= maxLevel; ++l )
      {
         edgeTables_.emplace_back();
         storage->forLocalCells( [&]( uint_t, const MacroCell& cell ) {
            edgeTables_.back().add( *storage, freeslip::edgeShellPoints( *storage, cell, l ), normal_function );
         } );
      }
   }
   void project( const P2Function< double >& u, const P2Function< double >& v, const P2Function< double >& w, uint_t level, DoFType flag ) const
   {
      p1Operator_.project( u.getVertexDoFFunction(), v.getVertexDoFFunction(), w.getVertexDoFFunction(), level, flag );
      ScopedTimer     timer( storage_->getTimingTree(), "Project" );
      const Selection sel   = u.effectiveFlag( flag ); // checked by the vertex projection
      const auto      masks = storage_->masksFor( sel, false, HYTEG_HIP_MASK_SHELL );
      storage_->forCellChunks( [&]( int first, int count ) {
         const auto us = u.edgeCellPointers( level, first, count ), vs = v.edgeCellPointers( level, first, count ),
                    ws = w.edgeCellPointers( level, first, count );
         hipCheck( hyteg_hip_p2_edge_project_normal_cells( count, us.data(), vs.data(), ws.data(), edgeTables_[level - minLevel_].data() + first,
                                                           (int) level, masks.data() + first, storage_->stream() ),
                   "P2ProjectNormalOperator::project" );
      } );
   }
   void project( const P2VectorFunction< double >& dst, uint_t level, DoFType flag ) const { project( dst[0], dst[1], dst[2], level, flag ); }
   void project( const P2P1TaylorHoodFunction< double >& dst, uint_t level, DoFType flag ) const { project( dst.uvw(), level, flag ); }

   std::shared_ptr< PrimitiveStorage > getStorage() const { return storage_; }
   uint_t                              getMinLevel() const { return minLevel_; }
   uint_t                              getMaxLevel() const { return maxLevel_; }

 private:
   P1ProjectNormalOperator               p1Operator_;
   std::shared_ptr< PrimitiveStorage >   storage_;
   uint_t                                minLevel_, maxLevel_;
   std::vector< freeslip::NormalTables > edgeTables_; // [level - minLevel]
};

// StrongFreeSlipWrapper.hpp:59-98: the operator followed by the projection (and, with PreProjection, preceded by it), which
// imposes free slip without touching the operator.  The levels of the temporary are those of the projection operator.
template < typename OpType, typename ProjOpType, bool PreProjection = false >
class StrongFreeSlipWrapper
{
 public:
   using srcType = typename OpType::srcType;
   using dstType = typename OpType::dstType;

   StrongFreeSlipWrapper( std::shared_ptr< OpType > op, std::shared_ptr< ProjOpType > projOp, DoFType projFlag )
   : op_( std::move( op ) )
   , projOp_( std::move( projOp ) )
   , projFlag_( projFlag )
   {
      if ( !op_ || !projOp_ )
         throw std::runtime_error( "StrongFreeSlipWrapper: needs an operator and a projection operator" );
      if ( PreProjection )
         tmp_ = std::make_shared< srcType >( "tmp", projOp_->getStorage(), projOp_->getMinLevel(), projOp_->getMaxLevel() );
   }

   void apply( const srcType& src, const dstType& dst, uint_t level, DoFType flag, UpdateType updateType = Replace ) const
   {
      if ( updateType != Replace )
         throw std::runtime_error( "Operator concatenation only supported for updateType Replace" );
      if ( PreProjection && projFlag_ != None )
      {
         tmp_->copyBoundaryConditionFromFunction( src ); // the projection selects its points with the condition of the function it is given
         tmp_->assign( { 1.0 }, { src }, level, All );
         projOp_->project( *tmp_, level, projFlag_ );
         op_->apply( *tmp_, dst, level, flag );
      }
      else
         op_->apply( src, dst, level, flag );
      if ( projFlag_ != None )
         projOp_->project( dst, level, projFlag_ );
   }
   std::shared_ptr< PrimitiveStorage > getStorage() const { return projOp_->getStorage(); }

 private:
   std::shared_ptr< OpType >     op_;
   std::shared_ptr< ProjOpType > projOp_;
   DoFType                       projFlag_;
   std::shared_ptr< srcType >    tmp_;
};

} // namespace hyteg
