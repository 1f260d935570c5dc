// lanes.hpp -- part of the C++ host layer above the C-ABI (see hyteg_host.hpp for the data model).
// LanePlanner: places launches whose arrays are known on a few in-order stream "lanes" so that independent launches overlap
// and dependent ones keep the order one stream would give them.  Pure host code, no HIP calls (PrimitiveStorage::LaneScope
// turns its answers into streams and events).  No counterpart in the reference, whose kernels are host loops.
#pragma once

#include <algorithm>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <unordered_map>
#include <vector>

namespace hyteg {

// Why: a level-8 apply loses ~2.7 us to the start and the tail of its grid and ~1.1 us to the barrier between two launches of
// one stream; independent applies issued alternately on two streams take 10.2-11.2 instead of 12.1-12.9 us each
// (profiles/r03_cell_streams.txt) -- the next launch ramps up while the last waves of the previous one drain.
//
// Model: a launch reads and writes whole arrays, named by their device base pointers.  Lane l is an in-order stream.  "Lane a
// waits for lane b" stands for an event recorded on b now and waited for by a: it orders everything issued on b SO FAR before
// everything issued on a FROM NOW ON.  synced_[a][b] counts the launches of b that a is ordered behind in this way (also
// through third lanes); a conflict with the i-th launch of b needs synced_[a][b] >= i, and only then is a wait handed out --
// never one per launch (two cross-stream events per apply cost more than the overlap gains, see PrimitiveStorage::SideChain).
//
// Choice of lane: the one that needs the fewest waits, ties to the least recently used.  A dependent chain therefore stays on
// one lane with no event at all, a ring of independent (src, dst) pairs alternates, and a ring that is revisited follows its
// own history: the second visit of a pair goes where the first one went.
class LanePlanner
{
 public:
   static constexpr int kMaxLanes = 8;

   explicit LanePlanner( int lanes = 2 ) { setLanes( lanes ); }

   void setLanes( int lanes )
   {
      if ( lanes < 1 || lanes > kMaxLanes )
         throw std::runtime_error( "LanePlanner: between 1 and " + std::to_string( kMaxLanes ) + " lanes" );
      lanes_ = lanes;
      reset();
   }
   int lanes() const { return lanes_; }

   // everything issued so far is ordered before everything that follows (the caller has joined the lanes)
   void reset()
   {
      arrays_.clear();
      for ( int a = 0; a < kMaxLanes; ++a )
      {
         issued_[a] = lastUse_[a] = 0;
         for ( int b = 0; b < kMaxLanes; ++b )
            synced_[a][b] = 0;
      }
      clock_ = 0;
   }

   struct Placement
   {
      int      lane;
      unsigned waits; // bit j: the lane waits for lane j (everything issued there so far) before this launch
   };

   Placement place( const void* const* reads, int nReads, const void* const* writes, int nWrites )
   {
      // the accesses this launch conflicts with: last write of everything it touches, reads since then of what it writes
      need_.clear();
      for ( int i = 0; i < nReads; ++i )
      {
         auto it = arrays_.find( reads[i] );
         if ( it != arrays_.end() && it->second.writeLane >= 0 )
            need_.push_back( { it->second.writeLane, it->second.writeIndex } );
      }
      for ( int i = 0; i < nWrites; ++i )
      {
         auto it = arrays_.find( writes[i] );
         if ( it == arrays_.end() )
            continue;
         if ( it->second.writeLane >= 0 )
            need_.push_back( { it->second.writeLane, it->second.writeIndex } );
         for ( int l = 0; l < lanes_; ++l )
            if ( it->second.readIndex[l] > 0 )
               need_.push_back( { l, it->second.readIndex[l] } );
      }
      int      best = 0, bestCount = kMaxLanes + 1;
      unsigned bestWaits = 0;
      for ( int a = 0; a < lanes_; ++a )
      {
         unsigned w = 0;
         for ( const Access& n : need_ )
            if ( n.lane != a && synced_[a][n.lane] < n.index )
               w |= 1u << n.lane;
         const int count = popcount( w );
         if ( count < bestCount || ( count == bestCount && lastUse_[a] < lastUse_[best] ) )
            best = a, bestCount = count, bestWaits = w;
      }
      for ( int b = 0; b < lanes_; ++b )
         if ( bestWaits & ( 1u << b ) )
         {
            // behind everything b has issued, and behind whatever b is behind
            synced_[best][b] = issued_[b];
            for ( int k = 0; k < lanes_; ++k )
               if ( k != best )
                  synced_[best][k] = std::max( synced_[best][k], synced_[b][k] );
         }
      const uint64_t index = ++issued_[best];
      lastUse_[best]       = ++clock_;
      for ( int i = 0; i < nReads; ++i )
         arrays_[reads[i]].readIndex[best] = index;
      for ( int i = 0; i < nWrites; ++i )
      {
         // the writer is ordered behind every earlier access, so whoever is ordered behind the writer is as well
         Array& A     = arrays_[writes[i]];
         A.writeLane  = best;
         A.writeIndex = index;
         for ( int l = 0; l < kMaxLanes; ++l )
            A.readIndex[l] = 0;
      }
      return { best, bestWaits };
   }

 private:
   struct Access
   {
      int      lane;
      uint64_t index; // 1-based position among the launches of its lane
   };
   struct Array
   {
      int      writeLane  = -1;
      uint64_t writeIndex = 0;
      uint64_t readIndex[kMaxLanes] = {}; // last read on each lane since the last write, 0 = none
   };
   static int popcount( unsigned w )
   {
      int n = 0;
      for ( ; w; w &= w - 1 )
         ++n;
      return n;
   }

   int                                      lanes_ = 2;
   uint64_t                                 issued_[kMaxLanes], lastUse_[kMaxLanes], synced_[kMaxLanes][kMaxLanes], clock_ = 0;
   std::unordered_map< const void*, Array > arrays_;
   std::vector< Access >                    need_;
};

// Grouping of a run of applies for the steps launch (hyteg_hip_p1_apply_cell_steps: up to 16 independent applies of one operator in
// one grid, so that a step starts while the waves of the one before it drain).  Step k of the run reads srcs[k] and writes dsts[k]
// (device base pointers of whole arrays).  A step conflicts with an earlier one if it writes an array that one reads or writes, or
// reads an array that one writes.  With one lane the groups are the maximal ones: consecutive steps join the group until it has
// maxGroup steps or the next step conflicts with one of its steps; that step starts the next group.  With several lanes a group
// must not swallow what the lanes would have overlapped: of the r conflict-free steps that follow the start of a group (looking
// at most maxGroup * lanes steps ahead) the group takes r / lanes and the next lanes - 1 groups as many (if they are
// conflict-free), so that every lane gets a launch out of the same steps -- a ring of 26 pairs gives groups of
// min( maxGroup, 13 ) on two lanes, 20 steps two groups of 10, a ring of 3 pairs single launches that alternate between the
// lanes as they did without groups.  Returns the group sizes in order (they sum to nsteps).  A ring with one pair, or a
// dependent chain dst[k] == src[k+1], degenerates to groups of one whatever the lanes.  Pure host code.
inline std::vector< int > planApplySteps( const void* const* srcs, const void* const* dsts, int nsteps, int maxGroup, int lanes = 1 )
{
   if ( maxGroup < 1 || lanes < 1 )
      throw std::runtime_error( "planApplySteps: group size and lane count must be at least 1" );
   std::vector< int > sizes;
   int                pending = 0, share = 0; // groups still owed to the other lanes by the last split, and its size
   for ( int begin = 0; begin < nsteps; )
   {
      const int window = std::min( nsteps - begin, maxGroup * lanes );
      int       r      = 1;
      for ( ; r < window; ++r )
      {
         const int k        = begin + r;
         bool      conflict = false;
         for ( int i = begin; i < k && !conflict; ++i )
            conflict = dsts[k] == srcs[i] || dsts[k] == dsts[i] || srcs[k] == dsts[i];
         if ( conflict )
            break;
      }
      int g;
      if ( pending > 0 ) // one of the equal shares of the split before: as large as that one, if that many steps are conflict-free
      {
         g = std::min( share, r );
         --pending;
      }
      else
      {
         g       = std::min( maxGroup, std::max( 1, r / lanes ) );
         share   = g;
         pending = lanes - 1;
      }
      sizes.push_back( g );
      begin += g;
   }
   return sizes;
}

} // namespace hyteg
