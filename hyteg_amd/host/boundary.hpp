// boundary.hpp -- part of the C++ host layer above the C-ABI (see hyteg_host.hpp for the data model).
// BoundaryUID, BoundaryCondition (src/hyteg/boundary/BoundaryConditions.{hpp,cpp}) and Selection, the pair of a DoFType flag and
// the boundary condition that gives it a meaning: what every mask of this layer is computed from.
#pragma once

#include "types.hpp"

namespace hyteg {

// Names one boundary of a BoundaryCondition (BoundaryConditions.hpp: BoundaryUID).  The id counts the boundaries of the
// condition that created it, from 1; id 0 is the boundary of every mesh flag that was given none.
struct BoundaryUID
{
   int         id = 0;
   std::string name;
   bool        operator==( const BoundaryUID& o ) const { return id == o.id && name == o.name; }
   bool        operator!=( const BoundaryUID& o ) const { return !( *this == o ); }
};

// Maps the mesh boundary flag of a macro-primitive to a DoFType (BoundaryCondition::getBoundaryType).  A value class: functions
// hold their own copy (Function::setBoundaryCondition).
class BoundaryCondition
{
 public:
   // BoundaryCondition::BoundaryCondition(): no boundary, every flag has the default type
   explicit BoundaryCondition( DoFType defaultType = Inner )
   : defaultType_( defaultType )
   {
      uids_.push_back( BoundaryUID{ 0, "Default" } );
   }
   // BoundaryCondition::create0123BC
   static BoundaryCondition create0123BC()
   {
      BoundaryCondition bc;
      bc.createDirichletBC( "Dirichlet", 1 );
      bc.createNeumannBC( "Neumann", 2 );
      bc.createFreeslipBC( "Freeslip", 3 );
      return bc;
   }
   // BoundaryCondition::createAllInnerBC
   static BoundaryCondition createAllInnerBC() { return BoundaryCondition( Inner ); }

   // BoundaryCondition::createDomainBC and its four shorthands.  A flag that had a boundary moves to the new one.
   BoundaryUID createDomainBC( const std::string& name, DoFType type, const std::vector< uint_t >& flags )
   {
      if ( type != Inner && type != DirichletBoundary && type != NeumannBoundary && type != FreeslipBoundary )
         throw std::runtime_error( "BoundaryCondition: a boundary has exactly one of the types Inner, Dirichlet, Neumann, Freeslip" );
      for ( const BoundaryUID& u : uids_ )
         if ( u.name == name )
            throw std::runtime_error( "BoundaryCondition: boundary name '" + name + "' is taken" );
      const BoundaryUID uid{ (int) uids_.size(), name };
      uids_.push_back( uid );
      uidTypes_.push_back( type );
      for ( uint_t f : flags )
         flagToUid_[f] = uid.id;
      return uid;
   }
   BoundaryUID createInnerBC( const std::string& name, const std::vector< uint_t >& flags ) { return createDomainBC( name, Inner, flags ); }
   BoundaryUID createDirichletBC( const std::string& name, const std::vector< uint_t >& flags ) { return createDomainBC( name, DirichletBoundary, flags ); }
   BoundaryUID createNeumannBC( const std::string& name, const std::vector< uint_t >& flags ) { return createDomainBC( name, NeumannBoundary, flags ); }
   BoundaryUID createFreeslipBC( const std::string& name, const std::vector< uint_t >& flags ) { return createDomainBC( name, FreeslipBoundary, flags ); }
   BoundaryUID createInnerBC( const std::string& name, uint_t flag ) { return createInnerBC( name, std::vector< uint_t >{ flag } ); }
   BoundaryUID createDirichletBC( const std::string& name, uint_t flag ) { return createDirichletBC( name, std::vector< uint_t >{ flag } ); }
   BoundaryUID createNeumannBC( const std::string& name, uint_t flag ) { return createNeumannBC( name, std::vector< uint_t >{ flag } ); }
   BoundaryUID createFreeslipBC( const std::string& name, uint_t flag ) { return createFreeslipBC( name, std::vector< uint_t >{ flag } ); }

   // BoundaryCondition::getBoundaryType
   DoFType getBoundaryType( uint_t flag ) const
   {
      auto it = flagToUid_.find( flag );
      return it == flagToUid_.end() ? defaultType_ : uidTypes_[(size_t) it->second - 1];
   }
   // BoundaryCondition::getBoundaryUIDFromMeshFlag
   const BoundaryUID& getBoundaryUIDFromMeshFlag( uint_t flag ) const
   {
      auto it = flagToUid_.find( flag );
      return uids_[it == flagToUid_.end() ? 0 : (size_t) it->second];
   }
   // the uid names a boundary of THIS condition (id and name): ids are small numbers that every condition hands out anew
   bool hasBoundary( const BoundaryUID& uid ) const { return uid.id >= 0 && (size_t) uid.id < uids_.size() && uids_[(size_t) uid.id] == uid; }
   DoFType getDefaultBoundaryType() const { return defaultType_; }
   // PrimitiveStorage::setBoundaryType: the boundary that `flag` belongs to changes its type
   void retype( uint_t flag, DoFType type )
   {
      auto it = flagToUid_.find( flag );
      if ( it == flagToUid_.end() )
         throw std::runtime_error( "BoundaryCondition::retype: the flag has no boundary" );
      uidTypes_[(size_t) it->second - 1] = type;
   }
   // no flag maps to anything but Inner
   bool allInner() const
   {
      if ( defaultType_ != Inner )
         return false;
      for ( const auto& fu : flagToUid_ )
         if ( uidTypes_[(size_t) fu.second - 1] != Inner )
            return false;
      return true;
   }
   bool operator==( const BoundaryCondition& o ) const
   {
      return defaultType_ == o.defaultType_ && flagToUid_ == o.flagToUid_ && uidTypes_ == o.uidTypes_ && uids_ == o.uids_;
   }
   bool operator!=( const BoundaryCondition& o ) const { return !( *this == o ); }

 private:
   DoFType                    defaultType_;
   std::vector< BoundaryUID > uids_;     // [id]
   std::vector< DoFType >     uidTypes_; // [id - 1]
   std::map< uint_t, int >    flagToUid_;
};

// What a kernel's point mask is computed from: a DoFType flag, the boundary condition that types the mesh flags (null: the
// storage's default one), and optionally one boundary of that condition (interpolate( expr, level, BoundaryUID )): then the
// points of the primitives whose flag belongs to that boundary are selected and `flag` is not looked at.
// A bare DoFType converts to an unresolved selection: the function it is handed to puts it under its own condition
// (effectiveFlag), the storage under the default one.  A resolved selection is taken as it is by everybody, which is how an
// operator makes its temporaries select the points of its destination (copyBCs in the reference).
struct Selection
{
   DoFType                                    flag = All;
   std::shared_ptr< const BoundaryCondition > bc;
   int                                        uid      = -1;
   bool                                       resolved = false;

   Selection( DoFType f = All, std::shared_ptr< const BoundaryCondition > b = nullptr, int boundaryUid = -1, bool isResolved = false )
   : flag( f )
   , bc( std::move( b ) )
   , uid( boundaryUid )
   , resolved( isResolved )
   {}
   // the points of a primitive with this mesh flag are selected; dflt: the storage's default condition
   bool selects( uint_t meshFlag, const BoundaryCondition& dflt ) const
   {
      const BoundaryCondition& c = bc ? *bc : dflt;
      if ( uid >= 0 )
         return c.getBoundaryUIDFromMeshFlag( meshFlag ).id == uid;
      return testFlag( c.getBoundaryType( meshFlag ), flag );
   }
   // same points on every storage with the same default condition
   bool operator==( const Selection& o ) const
   {
      return flag == o.flag && uid == o.uid && ( bc == o.bc || ( bc && o.bc && *bc == *o.bc ) );
   }
   bool operator!=( const Selection& o ) const { return !( *this == o ); }
};

} // namespace hyteg
