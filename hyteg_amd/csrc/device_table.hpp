// Device-resident tables that are built once per device and never freed: tile, brick and block lists, operator tables,
// zero-filled scratch.  One upload helper and one cache; every get_* of the library goes through them.
// First use allocates and uploads synchronously; later uses are a lookup under the cache's lock.
#pragma once

#include <functional>
#include <map>
#include <mutex>
#include <utility>
#include <vector>

#include "common.hpp"

namespace hyteg_hip {

// host vector -> device array (hipMalloc + synchronous hipMemcpy); an empty vector gives a null pointer
template < typename T >
int upload_table( const std::vector< T >& host, const T** dev )
{
   *dev = nullptr;
   if ( host.empty() )
      return HYTEG_HIP_OK;
   void* p = nullptr;
   HH_CHECK_HIP( hipMalloc( &p, host.size() * sizeof( T ) ) );
   HH_CHECK_HIP( hipMemcpy( p, host.data(), host.size() * sizeof( T ), hipMemcpyHostToDevice ) );
   *dev = static_cast< const T* >( p );
   return HYTEG_HIP_OK;
}

// `count` zero-initialised entries on the device
template < typename T >
int zeroed_table( size_t count, T** dev )
{
   void* p = nullptr;
   HH_CHECK_HIP( hipMalloc( &p, count * sizeof( T ) ) );
   HH_CHECK_HIP( hipMemset( p, 0, count * sizeof( T ) ) );
   *dev = static_cast< T* >( p );
   return HYTEG_HIP_OK;
}

// Entries by (current device, key).  get() calls build( Value& ) -- which returns a HYTEG_HIP_* code -- only on a miss and hands
// back a pointer to the cached entry; entries are neither moved nor freed, so the pointer stays valid.
template < typename Key, typename Value >
class DeviceTableCache
{
 public:
   template < typename Build >
   int get( const Key& key, Build&& build, const Value** out )
   {
      int dev = 0;
      HH_CHECK_HIP( hipGetDevice( &dev ) );
      return get_on( dev, key, build, out );
   }
   // the same for a caller that has already asked for the current device
   template < typename Build >
   int get_on( int dev, const Key& key, Build&& build, const Value** out )
   {
      std::lock_guard< std::mutex > lock( mtx_ );
      auto                          it = map_.find( std::make_pair( dev, key ) );
      if ( it == map_.end() )
      {
         Value     v{};
         const int rc = build( v );
         if ( rc != HYTEG_HIP_OK )
            return rc;
         it = map_.emplace( std::make_pair( dev, key ), std::move( v ) ).first;
      }
      *out = &it->second;
      return HYTEG_HIP_OK;
   }

 private:
   std::mutex                                  mtx_;
   std::map< std::pair< int, Key >, Value > map_;
};

// Device copy of an operator table that an entry point builds per call, by a key of doubles (the table itself for the P2
// constant-stencil sub-operators; cell coordinates and level at the seam of the generated elementwise operators).  build fills the
// host table on a miss.
int cached_operator_table( const std::vector< double >& key, const std::function< int( std::vector< double >& ) >& build, const double** dev_out );

} // namespace hyteg_hip
