// C facade of the C++ host layer (include/hyteg_host.h).  Exceptions become return codes.
#include "hyteg_host.hpp"

#include <variant>

#include "../../include/hyteg_host.h"

using namespace hyteg;

namespace {
thread_local std::string g_err;

struct StorageH
{
   std::shared_ptr< PrimitiveStorage > p;
};
struct FunctionH
{
   std::shared_ptr< P1Function< double > > p;
};
// the alternative's index is the form id of hyteg_host_operator_create (include/hyteg_host.h): 0 Laplace, 1 mass, 2-4 div x/y/z,
// 5-7 divT x/y/z, 8 PSPG
struct OperatorH
{
   std::variant< std::shared_ptr< P1ConstantLaplaceOperator >, std::shared_ptr< P1ConstantMassOperator >, std::shared_ptr< P1DivxOperator >,
                 std::shared_ptr< P1DivyOperator >, std::shared_ptr< P1DivzOperator >, std::shared_ptr< P1DivTxOperator >,
                 std::shared_ptr< P1DivTyOperator >, std::shared_ptr< P1DivTzOperator >, std::shared_ptr< P1PSPGOperator > >
             op;
   FunctionH invDiag; // borrowed view
};
struct SolverH
{
   std::shared_ptr< Solver< P1ConstantLaplaceOperator > > p;
};
struct P2FunctionH
{
   std::shared_ptr< P2Function< double > > p;
};
struct P2OperatorH
{
   std::shared_ptr< P2ElementwiseLaplaceOperator > p;
};
struct P2SolverH
{
   std::shared_ptr< Solver< P2ElementwiseLaplaceOperator > > p;
};

template < typename F >
int guarded( F&& fn )
{
   try
   {
      fn();
      return 0;
   } catch ( const std::exception& e )
   {
      g_err = e.what();
      P2PTransport::abortExchangesOfAllTransports(); // no plan stays "in flight" behind a failed operation
      return 1;
   } catch ( ... )
   {
      g_err = "unknown error";
      P2PTransport::abortExchangesOfAllTransports();
      return 1;
   }
}
PrimitiveStorage&      S( hh_storage_t s ) { return *static_cast< StorageH* >( s )->p; }
std::shared_ptr< PrimitiveStorage > SP( hh_storage_t s ) { return static_cast< StorageH* >( s )->p; }
P1Function< double >&  F( hh_function_t f ) { return *static_cast< FunctionH* >( f )->p; }
std::vector< std::reference_wrapper< const P1Function< double > > > refs( int n, const hh_function_t* fs )
{
   std::vector< std::reference_wrapper< const P1Function< double > > > r;
   for ( int i = 0; i < n; ++i )
      r.push_back( std::cref( F( fs[i] ) ) );
   return r;
}
// key = ( cls & 1 ) + 2 * dof_kind + 4 * ( cls >> 1 ): PrimitiveStorage::planKey
const ExchangePlan& exchangePlanOfKey( hh_storage_t s, int level, int key )
{
   int cls, dofKind;
   PrimitiveStorage::splitPlanKey( key, cls, dofKind );
   return S( s ).exchangePlan( level, cls, dofKind );
}
const ExchangePlan& devicePlanOfKey( hh_storage_t s, int level, int key )
{
   int cls, dofKind;
   PrimitiveStorage::splitPlanKey( key, cls, dofKind );
   return S( s ).devicePlan( level, cls, dofKind );
}
struct BoundaryConditionH
{
   BoundaryCondition bc;
};
BoundaryCondition& BC( hh_boundary_condition_t b )
{
   if ( !b )
      throw std::runtime_error( "null boundary condition" );
   return static_cast< BoundaryConditionH* >( b )->bc;
}
// the selection of a C call: the DoFType flag, or -- boundary_uid >= 0 -- one boundary of the function's condition
template < class Function >
Selection selectionOf( const Function& f, int boundaryUid, const char* boundaryName )
{
   return f.boundarySelection( BoundaryUID{ boundaryUid, boundaryName ? boundaryName : "" } );
}
P2Function< double >& F2( hh_p2function_t f ) { return *static_cast< P2FunctionH* >( f )->p; }
std::vector< std::reference_wrapper< const P2Function< double > > > refs2( int n, const hh_p2function_t* fs )
{
   std::vector< std::reference_wrapper< const P2Function< double > > > r;
   for ( int i = 0; i < n; ++i )
      r.push_back( std::cref( F2( fs[i] ) ) );
   return r;
}
// one device pass for the five numbers; over the ranks: one sum of two values, three maxima (min = -max( -x ), VertexDoFFunction.cpp:2053)
template < typename Function >
void reduceInto( const Function& f, int level, int flag, int mpiReduce, double* out )
{
   const auto r                  = f.reduceLocal( (uint_t) level, DoFType( flag ) );
   out[HYTEG_HIP_REDUCE_SUM]     = r.sum;
   out[HYTEG_HIP_REDUCE_SUM_ABS] = r.sumAbs;
   out[HYTEG_HIP_REDUCE_MIN]     = r.min;
   out[HYTEG_HIP_REDUCE_MAX]     = r.max;
   out[HYTEG_HIP_REDUCE_MAX_ABS] = r.maxMagnitude;
   const PrimitiveStorage& st    = *f.getStorage();
   if ( !mpiReduce || st.numRanks() == 1 )
      return;
   st.requireTransport( "reduce" ).allreduceSum( out + HYTEG_HIP_REDUCE_SUM, 2 );
   out[HYTEG_HIP_REDUCE_MIN]     = -st.allreduceMax( -out[HYTEG_HIP_REDUCE_MIN], "reduce" );
   out[HYTEG_HIP_REDUCE_MAX]     = st.allreduceMax( out[HYTEG_HIP_REDUCE_MAX], "reduce" );
   out[HYTEG_HIP_REDUCE_MAX_ABS] = st.allreduceMax( out[HYTEG_HIP_REDUCE_MAX_ABS], "reduce" );
}
// fn( A ) with the operator the handle holds
template < typename Fn >
void withOp( hh_operator_t op, Fn&& fn )
{
   std::visit( [&]( auto& p ) { fn( *p ); }, static_cast< OperatorH* >( op )->op );
}
// the loop of hyteg_host_operator_apply_cycle and _apply_cycle_timed: consecutive applies on different pairs are independent, they
// share launches (P1ConstantOperator::applyRun sees all the steps before it issues the first) and overlap on the storage's lanes
// (PrimitiveStorage::LaneScope)
void applyCycle( hh_operator_t op, int npairs, const hh_function_t* srcs, const hh_function_t* dsts, int level, int flag, int update, int first, int steps )
{
   PrimitiveStorage::LaneScope lanes( *F( srcs[0] ).getStorage() );
   std::vector< const P1Function< double >* > u( (size_t) steps ), d( (size_t) steps );
   for ( int k = 0; k < steps; ++k )
   {
      const int j   = ( first + k ) % npairs;
      u[(size_t) k] = &F( srcs[j] );
      d[(size_t) k] = &F( dsts[j] );
   }
   withOp( op, [&]( auto& A ) { A.applyRun( u, d, (uint_t) level, DoFType( flag ), update ? Add : Replace ); } );
   lanes.join();
}
// scalar smoother of an integer code: 0 weighted Jacobi, 1 Gauss-Seidel, 2 SOR, 3 mixed-precision Jacobi (P1 only: BASELINE config 5's
// "fp32 smoother"), 5 symmetric Gauss-Seidel, 6 symmetric SOR (4 is the Chebyshev smoother, which has entry points of its own); null for
// any other code, which each caller maps in its own way
template < class Op >
std::shared_ptr< Solver< Op > > scalarSmoother( int code, const std::shared_ptr< PrimitiveStorage >& storage, int minL, int maxL, double relax )
{
   if ( code == 0 )
      return std::make_shared< WeightedJacobiSmoother< Op > >( storage, (uint_t) minL, (uint_t) maxL, relax );
   if ( code == 1 )
      return std::make_shared< GaussSeidelSmoother< Op > >();
   if ( code == 2 )
      return std::make_shared< SORSmoother< Op > >( relax );
   if constexpr ( std::is_same< Op, P1ConstantLaplaceOperator >::value )
      if ( code == 3 )
         return std::make_shared< MixedPrecisionJacobiSmoother< Op > >( storage, (uint_t) minL, (uint_t) maxL, relax );
   if ( code == 5 )
      return std::make_shared< SymmetricGaussSeidelSmoother< Op > >();
   if ( code == 6 )
      return std::make_shared< SymmetricSORSmoother< Op > >( relax );
   return nullptr;
}
// the facade of a smoother on its own and of a preconditioned CG solver, for either operator
template < class Op, class Handle >
void smootherCreate( const char* who, hh_storage_t s, int minL, int maxL, int code, double relax, void** out )
{
   std::shared_ptr< Solver< Op > > sm = scalarSmoother< Op >( code, SP( s ), minL, maxL, relax );
   if ( code == -1 )
      sm = std::make_shared< IdentityPreconditioner< Op > >();
   if ( !sm )
      throw std::runtime_error( std::string( who ) + ": unknown smoother code" );
   *out = new Handle{ sm };
}
template < class Op, class Handle >
void cgCreatePreconditioned( const char* who, hh_storage_t s, int minL, int maxL, int maxIter, double tol, void* preconditioner, void** out )
{
   if ( !preconditioner || !static_cast< Handle* >( preconditioner )->p )
      throw std::runtime_error( std::string( who ) + ": needs a preconditioner" );
   // the solver shares ownership of the preconditioner: the caller may destroy its handle
   *out = new Handle{ std::make_shared< CGSolver< Op > >( SP( s ), (uint_t) minL, (uint_t) maxL, (uint_t) maxIter, tol, tol,
                                                          static_cast< Handle* >( preconditioner )->p ) };
}
template < class Op, class Handle >
void cgIterations( const char* who, void* solver, int* iterations )
{
   auto cg = std::dynamic_pointer_cast< CGSolver< Op > >( static_cast< Handle* >( solver )->p );
   if ( !cg )
      throw std::runtime_error( std::string( who ) + ": not a CG solver" );
   *iterations = (int) cg->getIterations();
}
// CG on the coarsest level of a multigrid solver
template < class Op >
std::shared_ptr< Solver< Op > > cgCoarse( const std::shared_ptr< PrimitiveStorage >& storage, int minL, int cgMaxIter, double cgTol )
{
   return std::make_shared< CGSolver< Op > >( storage, (uint_t) minL, (uint_t) minL, (uint_t) cgMaxIter, cgTol, cgTol );
}
template < class Op, class Restriction = P1toP1LinearRestriction, class Prolongation = P1toP1LinearProlongation, class... RestrictionArgs >
std::shared_ptr< Solver< Op > > makeGmg( const std::shared_ptr< PrimitiveStorage >& storage, std::shared_ptr< Solver< Op > > smoother,
                                         std::shared_ptr< Solver< Op > > coarse, int minL, int maxL, int pre, int post, int increment, CycleType cycle,
                                         RestrictionArgs... restrictionArgs )
{
   return std::make_shared< GeometricMultigridSolver< Op, Restriction, Prolongation > >(
       storage, smoother, coarse, std::make_shared< Restriction >( restrictionArgs... ), std::make_shared< Prolongation >(), (uint_t) minL, (uint_t) maxL,
       (uint_t) pre, (uint_t) post, (uint_t) increment, cycle );
}
CycleType cycleOf( int wcycle ) { return wcycle ? CycleType::WCYCLE : CycleType::VCYCLE; }
struct QuadraticProlongationH
{
   std::shared_ptr< P1toP1QuadraticProlongationThroughP2Injection > p;
};
// the cycle counts of hyteg_host_fmg_create / hyteg_host_p2_fmg_create: nCycles == 0 is the scalar constructor form (one count for
// every level), otherwise the counts are handed on as given and FullMultigridSolver checks their number
std::vector< uint_t > fmgCycles( const char* who, int minL, int maxL, const unsigned* cyclesPerLevel, int nCycles )
{
   if ( minL < 0 || maxL < minL || !cyclesPerLevel || nCycles < 0 )
      throw std::runtime_error( std::string( who ) + ": needs 0 <= min_level <= max_level and cycle counts" );
   if ( nCycles == 0 )
      return std::vector< uint_t >( (size_t) maxL + 1, (uint_t) cyclesPerLevel[0] );
   return std::vector< uint_t >( cyclesPerLevel, cyclesPerLevel + nCycles );
}
std::function< void( uint_t ) > levelCallback( hh_level_callback_t fn, void* user )
{
   if ( !fn )
      return []( uint_t ) {};
   return [fn, user]( uint_t level ) { fn( (uint64_t) level, user ); };
}
// borrowed view of a component: an aliasing pointer that shares ownership with the composite and points at the component
template < class T, class Owner >
std::shared_ptr< T > viewOf( const std::shared_ptr< Owner >& owner, const T& component )
{
   return std::shared_ptr< T >( owner, const_cast< T* >( &component ) );
}

// The two Stokes groups of the facade -- hyteg_host_stokes_* (P1-P1) and hyteg_host_th_* (P2-P1 Taylor-Hood) -- written once over the
// operator and the handle of a velocity component; the extern "C" functions forward to these.
template < class Operator, class VelocityH >
struct StokesFacade
{
   using Op = Operator;
   using Fn = typename Operator::srcType;
   struct FunctionHandle
   {
      std::shared_ptr< Fn > p;
      VelocityH             velocity[3]; // borrowed views of u, v, w
      FunctionH             pressure;    // and of p
   };
   struct OperatorHandle
   {
      std::shared_ptr< Op > p;
   };
   struct SolverHandle
   {
      std::shared_ptr< Solver< Op > > p;
   };
   static Fn&           fn( void* f ) { return *static_cast< FunctionHandle* >( f )->p; }
   static Op&           op( void* o ) { return *static_cast< OperatorHandle* >( o )->p; }
   static Solver< Op >& solver( void* s ) { return *static_cast< SolverHandle* >( s )->p; }

   static int functionCreate( hh_storage_t s, const char* name, int minL, int maxL, void** out )
   {
      return guarded( [&] {
         auto* h = new FunctionHandle{};
         h->p    = std::make_shared< Fn >( name, SP( s ), (uint_t) minL, (uint_t) maxL );
         *out    = h;
      } );
   }
   static void* velocityView( void* f, int k )
   {
      auto* h          = static_cast< FunctionHandle* >( f );
      h->velocity[k].p = viewOf( h->p, h->p->uvw()[(uint_t) k] );
      return &h->velocity[k];
   }
   static void* pressureView( void* f )
   {
      auto* h       = static_cast< FunctionHandle* >( f );
      h->pressure.p = viewOf( h->p, h->p->p() );
      return &h->pressure;
   }
   static int functionAssign( void* dst, int n, const double* scalars, void* const* fs, int level, int flag )
   {
      return guarded( [&] {
         typename Fn::Refs r;
         for ( int i = 0; i < n; ++i )
            r.push_back( std::cref( fn( fs[i] ) ) );
         fn( dst ).assign( std::vector< double >( scalars, scalars + n ), r, (uint_t) level, DoFType( flag ) );
      } );
   }
   static int functionDot( void* a, void* b, int level, int flag, double* out )
   {
      return guarded( [&] { *out = fn( a ).dotGlobal( fn( b ), (uint_t) level, DoFType( flag ) ); } );
   }
   static int operatorCreate( hh_storage_t s, int minL, int maxL, void** out )
   {
      return guarded( [&] { *out = new OperatorHandle{ std::make_shared< Op >( SP( s ), (uint_t) minL, (uint_t) maxL ) }; } );
   }
   static int operatorApply( void* o, void* src, void* dst, int level, int flag )
   {
      return guarded( [&] { op( o ).apply( fn( src ), fn( dst ), (uint_t) level, DoFType( flag ) ); } );
   }
   static int solverSolve( void* s, void* o, void* x, void* b, int level )
   {
      return guarded( [&] { solver( s ).solve( op( o ), fn( x ), fn( b ), (uint_t) level ); } );
   }
   template < class Handle >
   static int destroy( void* h )
   {
      return guarded( [&] { delete static_cast< Handle* >( h ); } );
   }
   // MinResSolver preconditioned with StokesPressureBlockPreconditioner< ., P1LumpedInvMassOperator >, as
   // apps/stokesSphere/StokesSphere.cpp:227-237 composes it
   static std::shared_ptr< Solver< Op > > pressureMinres( const std::shared_ptr< PrimitiveStorage >& storage, int minL, int maxL, int maxIter, double relTol )
   {
      auto prec = std::make_shared< StokesPressureBlockPreconditioner< Op, P1LumpedInvMassOperator > >( storage, (uint_t) minL, (uint_t) maxL );
      return std::make_shared< MinResSolver< Op > >( storage, (uint_t) minL, (uint_t) maxL, (uint_t) maxIter, relTol, 1e-16, prec );
   }
};
using P1P1 = StokesFacade< P1P1StokesOperator, FunctionH >;
using TH   = StokesFacade< P2P1TaylorHoodStokesOperator, P2FunctionH >;

// The strong free-slip group of the facade, written once over a Stokes facade and its projection operator: the wrapper with and
// without pre-projection (two types in C++, one handle with a switch here) and the MINRES solver of a wrapped operator.
template < class Facade, class Projection >
struct FreeSlipFacade
{
   using Op   = typename Facade::Op;
   using Post = StrongFreeSlipWrapper< Op, Projection, false >;
   using Both = StrongFreeSlipWrapper< Op, Projection, true >;
   struct ProjectionHandle
   {
      std::shared_ptr< Projection > p;
   };
   struct WrapperHandle
   {
      std::shared_ptr< Post > post;
      std::shared_ptr< Both > both;
   };
   struct SolverHandle
   {
      std::shared_ptr< MinResSolver< Post > > post;
      std::shared_ptr< MinResSolver< Both > > both;
   };
   // normal( user, xyz, n ) != 0: the callback failed (a Python exception is waiting on the other side)
   static int projectionCreate( hh_storage_t s, int minL, int maxL, hh_normal_callback_t normal, void* user, void** out )
   {
      return guarded( [&] {
         if ( !normal )
            throw std::runtime_error( "project_normal_create: needs a normal function" );
         auto fn = [normal, user]( const Point3D& x, Point3D& n ) {
            if ( normal( user, x.data(), n.data() ) != 0 )
               throw std::runtime_error( "project_normal_create: the normal function failed" );
         };
         *out = new ProjectionHandle{ std::make_shared< Projection >( SP( s ), (uint_t) minL, (uint_t) maxL, fn ) };
      } );
   }
   static Projection& projection( void* p ) { return *static_cast< ProjectionHandle* >( p )->p; }
   static int         wrapperCreate( void* op, void* proj, int flag, int preProjection, void** out )
   {
      return guarded( [&] {
         auto  A = static_cast< typename Facade::OperatorHandle* >( op )->p;
         auto  P = static_cast< ProjectionHandle* >( proj )->p;
         auto* h = new WrapperHandle{};
         if ( preProjection )
            h->both = std::make_shared< Both >( A, P, DoFType( flag ) );
         else
            h->post = std::make_shared< Post >( A, P, DoFType( flag ) );
         *out = h;
      } );
   }
   static int wrapperApply( void* w, void* src, void* dst, int level, int flag )
   {
      return guarded( [&] {
         auto* h = static_cast< WrapperHandle* >( w );
         if ( h->both )
            h->both->apply( Facade::fn( src ), Facade::fn( dst ), (uint_t) level, DoFType( flag ) );
         else
            h->post->apply( Facade::fn( src ), Facade::fn( dst ), (uint_t) level, DoFType( flag ) );
      } );
   }
   // preconditioner 0 identity, 1 pressure block (lumped inverse mass): both act as the identity on the velocity, so they keep a
   // projected vector projected.  The block-diagonal preconditioner smooths the velocity of the unwrapped operator and does not.
   template < class W >
   static std::shared_ptr< MinResSolver< W > > makeMinres( hh_storage_t s, int minL, int maxL, int maxIter, double relTol, int preconditioner )
   {
      std::shared_ptr< Solver< W > > prec;
      if ( preconditioner == 0 )
         prec = std::make_shared< IdentityPreconditioner< W > >();
      else if ( preconditioner == 1 )
         prec = std::make_shared< StokesPressureBlockPreconditioner< W, P1LumpedInvMassOperator > >( SP( s ), (uint_t) minL, (uint_t) maxL );
      else if ( preconditioner == 2 )
         throw std::runtime_error( "free-slip minres: the \"block\" preconditioner does not keep projected velocities projected; use "
                                   "\"identity\" or \"pressure\" with a StrongFreeSlipWrapper" );
      else
         throw std::runtime_error( "free-slip minres: unknown preconditioner" );
      return std::make_shared< MinResSolver< W > >( SP( s ), (uint_t) minL, (uint_t) maxL, (uint_t) maxIter, relTol, 1e-16, prec );
   }
   static int minresCreate( hh_storage_t s, int minL, int maxL, int maxIter, double relTol, int preconditioner, int preProjection, void** out )
   {
      return guarded( [&] {
         auto h = std::make_unique< SolverHandle >();
         if ( preProjection )
            h->both = makeMinres< Both >( s, minL, maxL, maxIter, relTol, preconditioner );
         else
            h->post = makeMinres< Post >( s, minL, maxL, maxIter, relTol, preconditioner );
         *out = h.release();
      } );
   }
   static int solve( void* solver, void* w, void* x, void* b, int level )
   {
      return guarded( [&] {
         auto* sh = static_cast< SolverHandle* >( solver );
         auto* wh = static_cast< WrapperHandle* >( w );
         if ( sh->both && wh->both )
            sh->both->solve( *wh->both, Facade::fn( x ), Facade::fn( b ), (uint_t) level );
         else if ( sh->post && wh->post )
            sh->post->solve( *wh->post, Facade::fn( x ), Facade::fn( b ), (uint_t) level );
         else
            throw std::runtime_error( "free-slip minres: solver and wrapper differ in pre_projection" );
      } );
   }
   static int iterations( void* solver, int* out )
   {
      return guarded( [&] {
         auto* sh = static_cast< SolverHandle* >( solver );
         *out     = (int) ( sh->both ? sh->both->getIterations() : sh->post->getIterations() );
      } );
   }
};
using P1FreeSlip = FreeSlipFacade< P1P1, P1ProjectNormalOperator >;
using THFreeSlip = FreeSlipFacade< TH, P2ProjectNormalOperator >;

// ChebyshevSmoother with its coefficients set up (one spectral radius for all levels, or one per level)
template < class Op >
std::shared_ptr< ChebyshevSmoother< Op > > makeChebyshev( hh_storage_t s, int minL, int maxL, int order, const double* radii, int nRadii, double upper,
                                                          double lower )
{
   if ( !radii || ( nRadii != 1 && nRadii != maxL - minL + 1 ) )
      throw std::runtime_error( "chebyshev: pass one spectral radius, or one per level" );
   auto sm = std::make_shared< ChebyshevSmoother< Op > >( SP( s ), (uint_t) minL, (uint_t) maxL );
   if ( nRadii == 1 )
      sm->setupCoefficients( (uint_t) order, radii[0], upper, lower );
   else
      sm->setupCoefficients( (uint_t) order, std::vector< double >( radii, radii + nRadii ), upper, lower );
   return sm;
}
} // namespace

extern "C" {

HYTEG_HOST_API const char* hyteg_host_last_error( void ) { return g_err.c_str(); }

HYTEG_HOST_API int hyteg_host_storage_from_gmsh( const char* path, int rank, int nranks, hh_storage_t* out )
{
   return guarded( [&] { *out = new StorageH{ std::make_shared< PrimitiveStorage >( MeshInfo::fromGmshFile( path ), rank, nranks ) }; } );
}
HYTEG_HOST_API int hyteg_host_storage_from_arrays( int nv, const double* xyz, int nc, const int* cells, int rank, int nranks, hh_storage_t* out )
{
   return guarded( [&] { *out = new StorageH{ std::make_shared< PrimitiveStorage >( MeshInfo::fromArrays( nv, xyz, nc, cells ), rank, nranks ) }; } );
}
HYTEG_HOST_API int hyteg_host_storage_destroy( hh_storage_t s )
{
   return guarded( [&] { delete static_cast< StorageH* >( s ); } );
}
HYTEG_HOST_API int hyteg_host_storage_counts( hh_storage_t s, int* c )
{
   return guarded( [&] {
      auto& st = S( s );
      c[0]     = (int) st.getCells().size();
      c[1]     = (int) st.getFaces().size();
      c[2]     = (int) st.getEdges().size();
      c[3]     = (int) st.getVertices().size();
      c[4]     = (int) st.getNumberOfLocalCells();
      c[5]     = st.numRanks();
   } );
}
HYTEG_HOST_API int hyteg_host_storage_local_cell( hh_storage_t s, int li, int* gid, double* coords12, double* nnc14 )
{
   return guarded( [&] {
      const MacroCell& c = S( s ).getLocalCell( (uint_t) li );
      if ( gid )
         *gid = c.id;
      if ( coords12 )
         for ( int v = 0; v < 4; ++v )
            for ( int r = 0; r < 3; ++r )
               coords12[3 * v + r] = c.coords[v][r];
      if ( nnc14 )
      {
         auto n = S( s ).numNeighborCells( c );
         std::copy( n.begin(), n.end(), nnc14 );
      }
   } );
}
HYTEG_HOST_API int hyteg_host_storage_mask( hh_storage_t s, int li, int flag, int owned, unsigned* mask )
{
   return guarded( [&] {
      const MacroCell& c = S( s ).getLocalCell( (uint_t) li );
      *mask              = owned ? S( s ).ownedMaskFor( c, DoFType( flag ) ) : S( s ).maskFor( c, DoFType( flag ) );
   } );
}
HYTEG_HOST_API int hyteg_host_storage_mask_bc( hh_storage_t s, int li, int flag, int owned, hh_boundary_condition_t bc, unsigned* mask )
{
   return guarded( [&] {
      const MacroCell& c = S( s ).getLocalCell( (uint_t) li );
      const Selection  sel( DoFType( flag ), bc ? std::make_shared< const BoundaryCondition >( BC( bc ) ) : nullptr, -1, true );
      *mask              = owned ? S( s ).ownedMaskFor( c, sel ) : S( s ).maskFor( c, sel );
   } );
}
HYTEG_HOST_API int hyteg_host_storage_set_mesh_boundary_flags_on_boundary( hh_storage_t s, unsigned long long flag_on_boundary,
                                                                           unsigned long long flag_inner, int highest_dimension_always_inner )
{
   return guarded( [&] { S( s ).setMeshBoundaryFlagsOnBoundary( (uint_t) flag_on_boundary, (uint_t) flag_inner, highest_dimension_always_inner != 0 ); } );
}
HYTEG_HOST_API int hyteg_host_storage_set_mesh_boundary_flags_inner( hh_storage_t s, unsigned long long flag_inner, int highest_dimension_always_inner )
{
   return guarded( [&] { S( s ).setMeshBoundaryFlagsInner( (uint_t) flag_inner, highest_dimension_always_inner != 0 ); } );
}
HYTEG_HOST_API int hyteg_host_storage_set_mesh_boundary_flags_by_vertex_location( hh_storage_t s, unsigned long long flag,
                                                                                  int ( *on_boundary )( void*, const double* ), void* user,
                                                                                  int all_vertices )
{
   return guarded( [&] {
      if ( !on_boundary )
         throw std::runtime_error( "set_mesh_boundary_flags_by_vertex_location: null predicate" );
      S( s ).setMeshBoundaryFlagsByVertexLocation( (uint_t) flag, [&]( const Point3D& x ) { return on_boundary( user, x.data() ) != 0; }, all_vertices != 0 );
   } );
}
HYTEG_HOST_API int hyteg_host_storage_set_mesh_boundary_flags_by_centroid_location( hh_storage_t s, unsigned long long flag,
                                                                                    int ( *on_boundary )( void*, const double* ), void* user )
{
   return guarded( [&] {
      if ( !on_boundary )
         throw std::runtime_error( "set_mesh_boundary_flags_by_centroid_location: null predicate" );
      S( s ).setMeshBoundaryFlagsByCentroidLocation( (uint_t) flag, [&]( const Point3D& x ) { return on_boundary( user, x.data() ) != 0; } );
   } );
}
HYTEG_HOST_API int hyteg_host_storage_set_mesh_boundary_flag( hh_storage_t s, int dim, int index, unsigned long long flag )
{
   return guarded( [&] {
      if ( index < 0 )
         throw std::runtime_error( "set_mesh_boundary_flag: negative index" );
      S( s ).setMeshBoundaryFlag( dim, (uint_t) index, (uint_t) flag );
   } );
}
HYTEG_HOST_API int hyteg_host_storage_primitive( hh_storage_t s, int dim, int index, int* nvertices, int* vertex_ids3, double* coords9,
                                                 unsigned long long* flag, int* on_boundary )
{
   return guarded( [&] {
      if ( index < 0 )
         throw std::runtime_error( "storage_primitive: negative index" );
      const MacroPrimitive& p = S( s ).primitive( dim, (uint_t) index );
      *nvertices              = (int) p.v.size();
      for ( uint_t k = 0; k < p.v.size(); ++k )
      {
         vertex_ids3[k] = p.v[k];
         for ( int r = 0; r < 3; ++r )
            coords9[3 * k + (uint_t) r] = S( s ).getVertexCoordinates( (uint_t) p.v[k] )[(uint_t) r];
      }
      *flag        = p.meshBoundaryFlag;
      *on_boundary = p.onBoundary ? 1 : 0;
   } );
}
HYTEG_HOST_API int hyteg_host_storage_boundary_classes( hh_storage_t s, int* count, unsigned long long* flags )
{
   return guarded( [&] {
      const auto& c = S( s ).boundaryClasses();
      *count        = (int) c.size();
      if ( flags )
         std::copy( c.begin(), c.end(), flags );
   } );
}
HYTEG_HOST_API int hyteg_host_boundary_condition_create( int preset, hh_boundary_condition_t* out )
{
   return guarded( [&] {
      if ( preset < 0 || preset > 2 )
         throw std::runtime_error( "boundary_condition_create: preset 0 (no boundary), 1 (create0123BC) or 2 (createAllInnerBC)" );
      *out = new BoundaryConditionH{ preset == 1 ? BoundaryCondition::create0123BC() :
                                                   ( preset == 2 ? BoundaryCondition::createAllInnerBC() : BoundaryCondition() ) };
   } );
}
HYTEG_HOST_API int hyteg_host_boundary_condition_destroy( hh_boundary_condition_t bc )
{
   return guarded( [&] { delete static_cast< BoundaryConditionH* >( bc ); } );
}
HYTEG_HOST_API int hyteg_host_boundary_condition_create_domain( hh_boundary_condition_t bc, const char* name, int dof_type, int nflags,
                                                                const unsigned long long* flags, int* uid )
{
   return guarded( [&] {
      std::vector< uint_t > f;
      for ( int i = 0; i < nflags; ++i )
         f.push_back( (uint_t) flags[i] );
      *uid = BC( bc ).createDomainBC( name ? name : "", DoFType( dof_type ), f ).id;
   } );
}
HYTEG_HOST_API int hyteg_host_boundary_condition_type( hh_boundary_condition_t bc, unsigned long long flag, int* dof_type )
{
   return guarded( [&] { *dof_type = (int) BC( bc ).getBoundaryType( (uint_t) flag ); } );
}
HYTEG_HOST_API int hyteg_host_boundary_condition_uid( hh_boundary_condition_t bc, unsigned long long flag, int* uid, char* name, int buflen )
{
   return guarded( [&] {
      const BoundaryUID& u = BC( bc ).getBoundaryUIDFromMeshFlag( (uint_t) flag );
      *uid                 = u.id;
      if ( name && buflen > 0 )
      {
         std::strncpy( name, u.name.c_str(), (size_t) buflen - 1 );
         name[buflen - 1] = 0;
      }
   } );
}
HYTEG_HOST_API int hyteg_host_boundary_condition_equal( hh_boundary_condition_t a, hh_boundary_condition_t b, int* equal )
{
   return guarded( [&] { *equal = BC( a ) == BC( b ) ? 1 : 0; } );
}
HYTEG_HOST_API int hyteg_host_storage_default_boundary_condition( hh_storage_t s, hh_boundary_condition_t* out )
{
   return guarded( [&] { *out = new BoundaryConditionH{ S( s ).getDefaultBoundaryCondition() }; } );
}
HYTEG_HOST_API int hyteg_host_function_set_boundary_condition( hh_function_t f, hh_boundary_condition_t bc )
{
   return guarded( [&] { F( f ).setBoundaryCondition( BC( bc ) ); } );
}
HYTEG_HOST_API int hyteg_host_function_boundary_condition( hh_function_t f, hh_boundary_condition_t* out )
{
   return guarded( [&] { *out = new BoundaryConditionH{ F( f ).getBoundaryCondition() }; } );
}
HYTEG_HOST_API int hyteg_host_function_interpolate_constant_on_boundary( hh_function_t f, double v, int level, int boundary_uid,
                                                                         const char* boundary_name )
{
   return guarded( [&] { F( f ).interpolate( v, (uint_t) level, selectionOf( F( f ), boundary_uid, boundary_name ) ); } );
}
HYTEG_HOST_API int hyteg_host_p2function_set_boundary_condition( hh_p2function_t f, hh_boundary_condition_t bc )
{
   return guarded( [&] { F2( f ).setBoundaryCondition( BC( bc ) ); } );
}
HYTEG_HOST_API int hyteg_host_p2function_boundary_condition( hh_p2function_t f, hh_boundary_condition_t* out )
{
   return guarded( [&] { *out = new BoundaryConditionH{ F2( f ).getBoundaryCondition() }; } );
}
HYTEG_HOST_API int hyteg_host_p2function_interpolate_constant_on_boundary( hh_p2function_t f, double v, int level, int boundary_uid,
                                                                           const char* boundary_name )
{
   return guarded( [&] { F2( f ).interpolate( v, (uint_t) level, selectionOf( F2( f ), boundary_uid, boundary_name ) ); } );
}
HYTEG_HOST_API int hyteg_host_storage_set_boundary_type( hh_storage_t s, int t )
{
   return guarded( [&] { S( s ).setBoundaryType( DoFType( t ) ); } );
}
HYTEG_HOST_API int hyteg_host_storage_set_stream( hh_storage_t s, void* stream )
{
   return guarded( [&] { S( s ).setStream( stream ); } );
}
HYTEG_HOST_API int hyteg_host_storage_set_batch_max_level( hh_storage_t s, int level )
{
   return guarded( [&] { S( s ).setBatchMaxLevel( level ); } );
}
HYTEG_HOST_API int hyteg_host_storage_set_apply_lanes( hh_storage_t s, int lanes )
{
   return guarded( [&] { S( s ).setApplyLanes( lanes ); } );
}
HYTEG_HOST_API int hyteg_host_storage_set_apply_steps( hh_storage_t s, int steps )
{
   return guarded( [&] { S( s ).setApplySteps( steps ); } );
}
HYTEG_HOST_API int hyteg_host_storage_steps_launches( hh_storage_t s, unsigned* count )
{
   return guarded( [&] { *count = S( s ).stepsLaunchesSeen(); } );
}
HYTEG_HOST_API int hyteg_host_storage_set_apply_cell_lanes_min( hh_storage_t s, int cells )
{
   return guarded( [&] { S( s ).setApplyCellLanesMin( cells ); } );
}
HYTEG_HOST_API int hyteg_host_storage_lanes_seen( hh_storage_t s, unsigned* mask )
{
   return guarded( [&] { *mask = S( s ).lanesSeen(); } );
}
HYTEG_HOST_API int hyteg_host_lane_plan( int lanes, int nsteps, const int* read_ptr, const unsigned long long* read_ids, const int* write_ptr,
                                         const unsigned long long* write_ids, int* lane_out, unsigned* waits_out )
{
   return guarded( [&] {
      if ( nsteps < 0 || ( nsteps > 0 && ( !read_ptr || !write_ptr || !lane_out || !waits_out ) ) )
         throw std::runtime_error( "lane_plan: null argument" );
      LanePlanner                 planner( lanes );
      std::vector< const void* > r, w;
      for ( int k = 0; k < nsteps; ++k )
      {
         r.clear(), w.clear();
         for ( int i = read_ptr[k]; i < read_ptr[k + 1]; ++i )
            r.push_back( reinterpret_cast< const void* >( (uintptr_t) read_ids[i] ) );
         for ( int i = write_ptr[k]; i < write_ptr[k + 1]; ++i )
            w.push_back( reinterpret_cast< const void* >( (uintptr_t) write_ids[i] ) );
         const auto p = planner.place( r.data(), (int) r.size(), w.data(), (int) w.size() );
         lane_out[k] = p.lane, waits_out[k] = p.waits;
      }
   } );
}
HYTEG_HOST_API int hyteg_host_apply_steps_plan( int npairs, const unsigned long long* src_ids, const unsigned long long* dst_ids, int first, int steps,
                                                int max_group, int lanes, int* sizes_out, int* ngroups_out )
{
   return guarded( [&] {
      if ( npairs < 1 || steps < 0 || first < 0 || !src_ids || !dst_ids || !ngroups_out || ( steps > 0 && !sizes_out ) )
         throw std::runtime_error( "apply_steps_plan: bad argument" );
      std::vector< const void* > u( (size_t) steps ), d( (size_t) steps );
      for ( int k = 0; k < steps; ++k )
      {
         const int j   = (int) ( ( (long long) first + k ) % npairs );
         u[(size_t) k] = reinterpret_cast< const void* >( (uintptr_t) src_ids[j] );
         d[(size_t) k] = reinterpret_cast< const void* >( (uintptr_t) dst_ids[j] );
      }
      const std::vector< int > sizes = planApplySteps( u.data(), d.data(), steps, max_group, lanes );
      std::copy( sizes.begin(), sizes.end(), sizes_out );
      *ngroups_out = (int) sizes.size();
   } );
}
HYTEG_HOST_API int hyteg_host_storage_use_rccl( hh_storage_t s, const unsigned char* unique_id )
{
   return guarded( [&] {
      if ( !unique_id )
         throw std::runtime_error( "storage_use_rccl: null unique id" );
      S( s ).useRccl( unique_id );
   } );
}
HYTEG_HOST_API int hyteg_host_storage_use_p2p( hh_storage_t s, size_t arena_bytes, unsigned char* handle, int* arena_kind )
{
   return guarded( [&] {
      if ( !handle )
         throw std::runtime_error( "storage_use_p2p: null handle buffer" );
      P2PTransport& T = S( s ).useP2P( arena_bytes );
      std::copy( T.handle().begin(), T.handle().end(), handle );
      if ( arena_kind )
         *arena_kind = T.arenaKind();
   } );
}
HYTEG_HOST_API int hyteg_host_storage_p2p_open( hh_storage_t s, const unsigned char* handles )
{
   return guarded( [&] {
      if ( !handles )
         throw std::runtime_error( "storage_p2p_open: null handles" );
      S( s ).p2p().openPeers( handles );
   } );
}
HYTEG_HOST_API int hyteg_host_storage_p2p_layout( hh_storage_t s, int level, int key, long long* offsets )
{
   return guarded( [&] {
      const auto& plan = devicePlanOfKey( s, level, key );
      const auto  o    = S( s ).p2p().layoutPlan( plan, level, key );
      if ( !o.empty() && !offsets )
         throw std::runtime_error( "storage_p2p_layout: null offsets" );
      std::copy( o.begin(), o.end(), offsets );
   } );
}
HYTEG_HOST_API int hyteg_host_storage_p2p_connect( hh_storage_t s, int level, int key, const long long* offsets )
{
   return guarded( [&] {
      const auto& plan = devicePlanOfKey( s, level, key );
      if ( !plan.peers.empty() && !offsets )
         throw std::runtime_error( "storage_p2p_connect: null offsets" );
      S( s ).p2p().connectPlan( plan, level, key, offsets );
   } );
}
HYTEG_HOST_API int hyteg_host_storage_drop_p2p( hh_storage_t s )
{
   return guarded( [&] { S( s ).dropP2P(); } );
}
HYTEG_HOST_API int hyteg_host_storage_check_transport( hh_storage_t s )
{
   return guarded( [&] { S( s ).checkTransport(); } );
}
HYTEG_HOST_API int hyteg_host_storage_allreduce_sum( hh_storage_t s, double* values, int n )
{
   return guarded( [&] {
      if ( S( s ).numRanks() > 1 )
         S( s ).requireTransport( "allreduce_sum" ).allreduceSum( values, n );
   } );
}
HYTEG_HOST_API int hyteg_host_storage_allreduce_max( hh_storage_t s, double* values, int n )
{
   return guarded( [&] {
      for ( int k = 0; k < n; ++k )
         values[k] = S( s ).allreduceMax( values[k], "allreduce_max" );
   } );
}
HYTEG_HOST_API int hyteg_host_storage_p1_number_of_dofs( hh_storage_t s, int level, int global, unsigned long long* count )
{
   return guarded( [&] { *count = S( s ).numberOfDoFs( (uint_t) level, 0, global != 0 ); } );
}
HYTEG_HOST_API int hyteg_host_storage_p2_number_of_dofs( hh_storage_t s, int level, int global, unsigned long long* count )
{
   return guarded( [&] { *count = S( s ).numberOfDoFs( (uint_t) level, 0, global != 0 ) + S( s ).numberOfDoFs( (uint_t) level, 1, global != 0 ); } );
}
HYTEG_HOST_API int hyteg_host_storage_enable_timing( hh_storage_t s, int on, int synchronize )
{
   return guarded( [&] { S( s ).enableTiming( on != 0, synchronize != 0 ); } );
}
HYTEG_HOST_API int hyteg_host_storage_timing_json( hh_storage_t s, char* buf, size_t buflen, size_t* needed )
{
   return guarded( [&] {
      if ( !S( s ).getTimingTree() )
         throw std::runtime_error( "storage_timing_json: timing is not enabled" );
      const std::string j = S( s ).getTimingTree()->toJSON();
      if ( needed )
         *needed = j.size() + 1;
      if ( buf && buflen > 0 )
         snprintf( buf, buflen, "%s", j.c_str() );
   } );
}
HYTEG_HOST_API int hyteg_host_storage_timing_reset( hh_storage_t s )
{
   return guarded( [&] {
      if ( S( s ).getTimingTree() )
         S( s ).getTimingTree()->reset();
   } );
}
HYTEG_HOST_API int hyteg_host_storage_transport_name( hh_storage_t s, char* buf, int buflen )
{
   return guarded( [&] {
      const char* n = S( s ).transport() ? S( s ).transport()->name() : "none";
      snprintf( buf, (size_t) buflen, "%s", n );
   } );
}
HYTEG_HOST_API int hyteg_host_storage_set_hooks( hh_storage_t s, int ( *exb )( void*, int, int ), int ( *exe )( void*, int, int ),
                                                 int ( *ar )( void*, double*, int ), void* user )
{
   return guarded( [&] {
      CommHooks h;
      h.exchangeBegin = exb;
      h.exchangeEnd   = exe;
      h.allreduceSum = ar;
      h.user         = user;
      S( s ).setCommHooks( h );
   } );
}
// key = ( cls & 1 ) + 2 * dof_kind + 4 * ( cls >> 1 ) (dof_kind 0: vertex DoFs, 1: edge DoFs of P2 functions)
HYTEG_HOST_API int hyteg_host_plan_sizes( hh_storage_t s, int level, int key, int* sizes )
{
   return guarded( [&] {
      const auto& P = exchangePlanOfKey( s, level, key );
      sizes[0]      = P.ngroups();
      sizes[1]      = (int) P.entryBuf.size();
      sizes[2]      = (int) P.peers.size();
      sizes[3]      = P.totalSend();
      sizes[4]      = P.totalRecv();
   } );
}
HYTEG_HOST_API int hyteg_host_plan_export( hh_storage_t s, int level, int key, int* gp, int* eb, int* eo, int* peers, int* sc, int* rc, int* sb, int* so )
{
   return guarded( [&] {
      const auto& P = exchangePlanOfKey( s, level, key );
      std::copy( P.groupPtr.begin(), P.groupPtr.end(), gp );
      std::copy( P.entryBuf.begin(), P.entryBuf.end(), eb );
      std::copy( P.entryOff.begin(), P.entryOff.end(), eo );
      std::copy( P.peers.begin(), P.peers.end(), peers );
      std::copy( P.sendCount.begin(), P.sendCount.end(), sc );
      std::copy( P.recvCount.begin(), P.recvCount.end(), rc );
      std::copy( P.sendBuf.begin(), P.sendBuf.end(), sb );
      std::copy( P.sendOff.begin(), P.sendOff.end(), so );
   } );
}
HYTEG_HOST_API int hyteg_host_plan_register_buffers( hh_storage_t s, int level, int cls, double* send, double* recv )
{
   return guarded( [&] { S( s ).registerCommBuffers( level, cls, send, recv ); } );
}

HYTEG_HOST_API int hyteg_host_function_create( hh_storage_t s, const char* name, int minL, int maxL, hh_function_t* out )
{
   return guarded( [&] {
      *out = new FunctionH{ std::make_shared< P1Function< double > >( name, SP( s ), (uint_t) minL, (uint_t) maxL ) };
   } );
}
HYTEG_HOST_API int hyteg_host_function_destroy( hh_function_t f )
{
   return guarded( [&] { delete static_cast< FunctionH* >( f ); } );
}
HYTEG_HOST_API int hyteg_host_function_cell_pointer( hh_function_t f, int c, int level, double** p )
{
   return guarded( [&] { *p = F( f ).getCellPointer( (uint_t) c, (uint_t) level ); } );
}
HYTEG_HOST_API int hyteg_host_function_upload_cell( hh_function_t f, int c, int level, const double* host )
{
   return guarded( [&] { F( f ).copyCellFromHost( (uint_t) c, (uint_t) level, host ); } );
}
HYTEG_HOST_API int hyteg_host_function_download_cell( hh_function_t f, int c, int level, double* host )
{
   return guarded( [&] { F( f ).copyCellToHost( (uint_t) c, (uint_t) level, host ); } );
}
HYTEG_HOST_API int hyteg_host_function_interpolate_constant( hh_function_t f, double v, int level, int flag )
{
   return guarded( [&] { F( f ).interpolate( v, (uint_t) level, DoFType( flag ) ); } );
}
HYTEG_HOST_API int hyteg_host_function_assign( hh_function_t dst, int n, const double* sc, const hh_function_t* srcs, int level, int flag )
{
   return guarded( [&] { F( dst ).assign( std::vector< double >( sc, sc + n ), refs( n, srcs ), (uint_t) level, DoFType( flag ) ); } );
}
HYTEG_HOST_API int hyteg_host_function_add( hh_function_t dst, int n, const double* sc, const hh_function_t* srcs, int level, int flag )
{
   return guarded( [&] { F( dst ).add( std::vector< double >( sc, sc + n ), refs( n, srcs ), (uint_t) level, DoFType( flag ) ); } );
}
HYTEG_HOST_API int hyteg_host_function_mult_elementwise( hh_function_t dst, int n, const hh_function_t* srcs, int level, int flag )
{
   return guarded( [&] { F( dst ).multElementwise( refs( n, srcs ), (uint_t) level, DoFType( flag ) ); } );
}
HYTEG_HOST_API int hyteg_host_function_dot( hh_function_t a, hh_function_t b, int level, int flag, int global, double* result )
{
   return guarded( [&] {
      *result = global ? F( a ).dotGlobal( F( b ), (uint_t) level, DoFType( flag ) ) : F( a ).dotLocal( F( b ), (uint_t) level, DoFType( flag ) );
   } );
}
HYTEG_HOST_API int hyteg_host_p1_reduce( hh_function_t f, int level, int flag, int mpi_reduce, double* out )
{
   return guarded( [&] { reduceInto( F( f ), level, flag, mpi_reduce, out ); } );
}
HYTEG_HOST_API int hyteg_host_function_sum_shared( hh_function_t f, int level, int flag )
{
   return guarded( [&] { F( f ).sumSharedCopies( (uint_t) level, DoFType( flag ) ); } );
}
HYTEG_HOST_API int hyteg_host_function_set_all_inner( hh_function_t f, int on )
{
   return guarded( [&] { F( f ).setBoundaryConditionAllInner( on != 0 ); } );
}
HYTEG_HOST_API int hyteg_host_function_sync_shared( hh_function_t f, int level, int flag )
{
   return guarded( [&] { F( f ).syncSharedCopies( (uint_t) level, DoFType( flag ) ); } );
}

HYTEG_HOST_API int hyteg_host_operator_create( hh_storage_t s, int minL, int maxL, int form, hh_operator_t* out )
{
   return guarded( [&] {
      if ( form < 0 || form > 8 )
         throw std::runtime_error( "operator_create: unknown form id" );
      auto         h       = std::make_unique< OperatorH >();
      auto         storage = SP( s );
      const uint_t a = (uint_t) minL, b = (uint_t) maxL;
      switch ( form )
      {
      case 0: h->op = std::make_shared< P1ConstantLaplaceOperator >( storage, a, b ); break;
      case 1: h->op = std::make_shared< P1ConstantMassOperator >( storage, a, b ); break;
      case 2: h->op = std::make_shared< P1DivxOperator >( storage, a, b ); break;
      case 3: h->op = std::make_shared< P1DivyOperator >( storage, a, b ); break;
      case 4: h->op = std::make_shared< P1DivzOperator >( storage, a, b ); break;
      case 5: h->op = std::make_shared< P1DivTxOperator >( storage, a, b ); break;
      case 6: h->op = std::make_shared< P1DivTyOperator >( storage, a, b ); break;
      case 7: h->op = std::make_shared< P1DivTzOperator >( storage, a, b ); break;
      default: h->op = std::make_shared< P1PSPGOperator >( storage, a, b ); break;
      }
      *out = h.release();
   } );
}
HYTEG_HOST_API int hyteg_host_operator_destroy( hh_operator_t op )
{
   return guarded( [&] { delete static_cast< OperatorH* >( op ); } );
}
HYTEG_HOST_API int hyteg_host_operator_stencils( hh_operator_t op, int gc, int level, double* inner15, double* slots210 )
{
   return guarded( [&] {
      withOp( op, [&]( auto& A ) {
         const auto& st = A.getCellStencils( gc, (uint_t) level );
         std::copy( st.inner, st.inner + 15, inner15 );
         std::copy( &st.slots[0][0], &st.slots[0][0] + 210, slots210 );
      } );
   } );
}
HYTEG_HOST_API int hyteg_host_operator_apply( hh_operator_t op, hh_function_t src, hh_function_t dst, int level, int flag, int update )
{
   return guarded( [&] { withOp( op, [&]( auto& A ) { A.apply( F( src ), F( dst ), (uint_t) level, DoFType( flag ), update ? Add : Replace ); } ); } );
}
HYTEG_HOST_API int hyteg_host_operator_apply_cycle( hh_operator_t op, int npairs, const hh_function_t* srcs, const hh_function_t* dsts, int level,
                                                    int flag, int update, int first, int steps )
{
   return guarded( [&] {
      if ( steps > 0 && npairs > 0 )
         applyCycle( op, npairs, srcs, dsts, level, flag, update, first, steps );
   } );
}
HYTEG_HOST_API int hyteg_host_operator_apply_cycle_timed( hh_operator_t op, int npairs, const hh_function_t* srcs, const hh_function_t* dsts,
                                                          int level, int flag, int update, int first, int steps, void* evStart, void* evStop )
{
   // the same loop between two timing events of the C-ABI, recorded on the storage's stream directly before the first and after
   // the last apply (a measurement harness's bracket without its own call overhead inside)
   return guarded( [&] {
      if ( steps <= 0 || npairs <= 0 )
         return;
      hyteg_hip_stream_t stream = F( srcs[0] ).getStorage()->stream();
      if ( evStart )
         hipCheck( hyteg_hip_event_record( evStart, stream ), "apply_cycle_timed: record" );
      // evStart in front of the fork, evStop behind the join: both on the storage's stream, the lanes in between
      applyCycle( op, npairs, srcs, dsts, level, flag, update, first, steps );
      if ( evStop )
         hipCheck( hyteg_hip_event_record( evStop, stream ), "apply_cycle_timed: record" );
   } );
}
HYTEG_HOST_API int hyteg_host_operator_smooth_jac( hh_operator_t op, hh_function_t dst, hh_function_t rhs, hh_function_t src, double relax, int level, int flag )
{
   return guarded( [&] { withOp( op, [&]( auto& A ) { A.smooth_jac( F( dst ), F( rhs ), F( src ), relax, (uint_t) level, DoFType( flag ) ); } ); } );
}
HYTEG_HOST_API int hyteg_host_operator_smooth_sor( hh_operator_t op, hh_function_t dst, hh_function_t rhs, double relax, int level, int flag, int backwards )
{
   return guarded( [&] { withOp( op, [&]( auto& A ) { A.smooth_sor( F( dst ), F( rhs ), relax, (uint_t) level, DoFType( flag ), backwards != 0 ); } ); } );
}
HYTEG_HOST_API int hyteg_host_operator_smooth_sor_many( hh_operator_t op, int n, const hh_function_t* dsts, const hh_function_t* rhss, double relax,
                                                        int level, int flag, int backwards )
{
   return guarded( [&] {
      std::vector< std::reference_wrapper< const P1Function< double > > > xs, bs;
      for ( int k = 0; k < n; ++k )
      {
         xs.push_back( std::cref( F( dsts[k] ) ) );
         bs.push_back( std::cref( F( rhss[k] ) ) );
      }
      withOp( op, [&]( auto& A ) { A.smooth_sor_many( xs, bs, relax, (uint_t) level, DoFType( flag ), backwards != 0 ); } );
   } );
}
HYTEG_HOST_API int hyteg_host_operator_compute_inverse_diagonal( hh_operator_t op )
{
   return guarded( [&] { withOp( op, []( auto& A ) { A.computeInverseDiagonalOperatorValues(); } ); } );
}
HYTEG_HOST_API int hyteg_host_operator_inverse_diagonal( hh_operator_t op, hh_function_t* out )
{
   return guarded( [&] {
      auto* h = static_cast< OperatorH* >( op );
      withOp( op, [&]( auto& A ) { h->invDiag.p = A.getInverseDiagonalValues(); } );
      *out = &h->invDiag;
   } );
}

// ---- the generated elementwise operator class (module hyteg_operators): P1ElementwiseDiffusion ----
struct ElementwiseH
{
   std::shared_ptr< operatorgeneration::P1ElementwiseDiffusion > p;
   FunctionH                                                     invDiag; // borrowed view
};
HYTEG_HOST_API int hyteg_host_elementwise_create( hh_storage_t s, int minL, int maxL, hh_elementwise_t* out )
{
   return guarded( [&] {
      auto* h = new ElementwiseH{};
      h->p    = std::make_shared< operatorgeneration::P1ElementwiseDiffusion >( SP( s ), (uint_t) minL, (uint_t) maxL );
      *out    = h;
   } );
}
HYTEG_HOST_API int hyteg_host_elementwise_destroy( hh_elementwise_t op )
{
   return guarded( [&] { delete static_cast< ElementwiseH* >( op ); } );
}
HYTEG_HOST_API int hyteg_host_elementwise_apply( hh_elementwise_t op, hh_function_t src, hh_function_t dst, int level, int flag, int update )
{
   return guarded( [&] { static_cast< ElementwiseH* >( op )->p->apply( F( src ), F( dst ), (uint_t) level, DoFType( flag ), update ? Add : Replace ); } );
}
HYTEG_HOST_API int hyteg_host_elementwise_compute_inverse_diagonal( hh_elementwise_t op )
{
   return guarded( [&] { static_cast< ElementwiseH* >( op )->p->computeInverseDiagonalOperatorValues(); } );
}
HYTEG_HOST_API int hyteg_host_elementwise_inverse_diagonal( hh_elementwise_t op, hh_function_t* out )
{
   return guarded( [&] {
      auto* h      = static_cast< ElementwiseH* >( op );
      h->invDiag.p = h->p->getInverseDiagonalValues();
      *out         = &h->invDiag;
   } );
}
HYTEG_HOST_API int hyteg_host_elementwise_smooth_jac( hh_elementwise_t op, hh_function_t dst, hh_function_t rhs, hh_function_t src, double relax,
                                                      int level, int flag )
{
   return guarded( [&] { static_cast< ElementwiseH* >( op )->p->smooth_jac( F( dst ), F( rhs ), F( src ), relax, (uint_t) level, DoFType( flag ) ); } );
}

// ---- the generated variable-coefficient operator: P1ElementwiseDivKGrad, and the solvers instantiated for it ----
using DivKGrad = operatorgeneration::P1ElementwiseDivKGrad;
struct DivKGradH
{
   std::shared_ptr< P1Function< double > > k; // the operator holds a reference: the handle keeps the function alive
   std::shared_ptr< DivKGrad >             p;
   FunctionH                               invDiag; // borrowed view
};
struct DivKGradSolverH
{
   std::shared_ptr< Solver< DivKGrad > > p;
};
static DivKGrad& DK( hh_divkgrad_t op )
{
   if ( !op )
      throw std::runtime_error( "null divkgrad operator" );
   return *static_cast< DivKGradH* >( op )->p;
}
HYTEG_HOST_API int hyteg_host_divkgrad_create( hh_storage_t s, int minL, int maxL, hh_function_t k, hh_divkgrad_t* out )
{
   return guarded( [&] {
      if ( !k || minL < 0 || maxL < minL )
         throw std::runtime_error( "divkgrad_create: needs a coefficient function and 0 <= min_level <= max_level" );
      auto* h = new DivKGradH{};
      h->k    = static_cast< FunctionH* >( k )->p;
      try
      {
         h->p = std::make_shared< DivKGrad >( SP( s ), (uint_t) minL, (uint_t) maxL, *h->k );
      } catch ( ... )
      {
         delete h;
         throw;
      }
      *out = h;
   } );
}
HYTEG_HOST_API int hyteg_host_divkgrad_destroy( hh_divkgrad_t op )
{
   return guarded( [&] { delete static_cast< DivKGradH* >( op ); } );
}
HYTEG_HOST_API int hyteg_host_divkgrad_apply( hh_divkgrad_t op, hh_function_t src, hh_function_t dst, int level, int flag, int update )
{
   return guarded( [&] { DK( op ).apply( F( src ), F( dst ), (uint_t) level, DoFType( flag ), update ? Add : Replace ); } );
}
HYTEG_HOST_API int hyteg_host_divkgrad_compute_inverse_diagonal( hh_divkgrad_t op )
{
   return guarded( [&] { DK( op ).computeInverseDiagonalOperatorValues(); } );
}
HYTEG_HOST_API int hyteg_host_divkgrad_inverse_diagonal( hh_divkgrad_t op, hh_function_t* out )
{
   return guarded( [&] {
      auto* h      = static_cast< DivKGradH* >( op );
      h->invDiag.p = DK( op ).getInverseDiagonalValues();
      *out         = &h->invDiag;
   } );
}
HYTEG_HOST_API int hyteg_host_divkgrad_smooth_jac( hh_divkgrad_t op, hh_function_t dst, hh_function_t rhs, hh_function_t src, double relax, int level,
                                                   int flag )
{
   return guarded( [&] { DK( op ).smooth_jac( F( dst ), F( rhs ), F( src ), relax, (uint_t) level, DoFType( flag ) ); } );
}
HYTEG_HOST_API int hyteg_host_divkgrad_residual( hh_divkgrad_t op, hh_function_t x, hh_function_t b, hh_function_t r, int level, int flag )
{
   return guarded( [&] { DK( op ).residual( F( x ), F( b ), F( r ), (uint_t) level, DoFType( flag ) ); } );
}
HYTEG_HOST_API int hyteg_host_divkgrad_set_fused( hh_divkgrad_t op, int on )
{
   return guarded( [&] { DK( op ).setFused( on != 0 ); } );
}
HYTEG_HOST_API int hyteg_host_divkgrad_cg_create( hh_storage_t s, int minL, int maxL, int maxIter, double tol, hh_divkgrad_solver_t preconditioner,
                                                  hh_divkgrad_solver_t* out )
{
   return guarded( [&] {
      if ( preconditioner )
         cgCreatePreconditioned< DivKGrad, DivKGradSolverH >( "divkgrad_cg_create", s, minL, maxL, maxIter, tol, preconditioner, out );
      else
         *out = new DivKGradSolverH{ std::make_shared< CGSolver< DivKGrad > >( SP( s ), (uint_t) minL, (uint_t) maxL, (uint_t) maxIter, tol, tol ) };
   } );
}
HYTEG_HOST_API int hyteg_host_divkgrad_cg_iterations( hh_divkgrad_solver_t solver, int* iterations )
{
   return guarded( [&] { cgIterations< DivKGrad, DivKGradSolverH >( "divkgrad_cg_iterations", solver, iterations ); } );
}
// the operator has no Gauss-Seidel sweep: weighted Jacobi (0) and the identity (-1)
static std::shared_ptr< Solver< DivKGrad > > divkgradSmoother( hh_storage_t s, int minL, int maxL, int code, double relax )
{
   if ( code == 0 )
      return std::make_shared< WeightedJacobiSmoother< DivKGrad > >( SP( s ), (uint_t) minL, (uint_t) maxL, relax );
   if ( code == -1 )
      return std::make_shared< IdentityPreconditioner< DivKGrad > >();
   throw std::runtime_error( "divkgrad_smoother_create: smoother 0 (weighted Jacobi) or -1 (identity)" );
}
HYTEG_HOST_API int hyteg_host_divkgrad_smoother_create( hh_storage_t s, int minL, int maxL, int smoother, double relax, hh_divkgrad_solver_t* out )
{
   return guarded( [&] { *out = new DivKGradSolverH{ divkgradSmoother( s, minL, maxL, smoother, relax ) }; } );
}
HYTEG_HOST_API int hyteg_host_divkgrad_gmg_create( hh_storage_t s, int minL, int maxL, double relax, int pre, int post, int wcycle, int cgMaxIter,
                                                   double cgTol, hh_divkgrad_solver_t* out )
{
   return guarded( [&] {
      *out = new DivKGradSolverH{ makeGmg< DivKGrad >( SP( s ), divkgradSmoother( s, minL, maxL, 0, relax ),
                                                       cgCoarse< DivKGrad >( SP( s ), minL, cgMaxIter, cgTol ), minL, maxL, pre, post, 0,
                                                       cycleOf( wcycle ) ) };
   } );
}
HYTEG_HOST_API int hyteg_host_divkgrad_chebyshev_estimate_radius( hh_divkgrad_t op, int level, int maxIter, hh_function_t x, hh_function_t tmp,
                                                                  double* radius )
{
   return guarded( [&] { *radius = chebyshev::estimateRadius( DK( op ), (uint_t) level, (uint_t) maxIter, F( x ).getStorage(), F( x ), F( tmp ) ); } );
}
HYTEG_HOST_API int hyteg_host_divkgrad_chebyshev_create( hh_storage_t s, int minL, int maxL, int order, const double* radii, int nRadii, double upper,
                                                         double lower, hh_divkgrad_solver_t* out )
{
   return guarded( [&] { *out = new DivKGradSolverH{ makeChebyshev< DivKGrad >( s, minL, maxL, order, radii, nRadii, upper, lower ) }; } );
}
HYTEG_HOST_API int hyteg_host_divkgrad_gmg_create_chebyshev( hh_storage_t s, int minL, int maxL, int order, const double* radii, int nRadii,
                                                             double upper, double lower, int pre, int post, int wcycle, int cgMaxIter, double cgTol,
                                                             hh_divkgrad_solver_t* out )
{
   return guarded( [&] {
      std::shared_ptr< Solver< DivKGrad > > sm = makeChebyshev< DivKGrad >( s, minL, maxL, order, radii, nRadii, upper, lower );
      *out = new DivKGradSolverH{ makeGmg< DivKGrad >( SP( s ), sm, cgCoarse< DivKGrad >( SP( s ), minL, cgMaxIter, cgTol ), minL, maxL, pre, post, 0,
                                                       cycleOf( wcycle ) ) };
   } );
}
HYTEG_HOST_API int hyteg_host_divkgrad_solver_solve( hh_divkgrad_solver_t solver, hh_divkgrad_t op, hh_function_t x, hh_function_t b, int level )
{
   return guarded( [&] { static_cast< DivKGradSolverH* >( solver )->p->solve( DK( op ), F( x ), F( b ), (uint_t) level ); } );
}
HYTEG_HOST_API int hyteg_host_divkgrad_solver_destroy( hh_divkgrad_solver_t solver )
{
   return guarded( [&] { delete static_cast< DivKGradSolverH* >( solver ); } );
}

HYTEG_HOST_API int hyteg_host_restrict( hh_function_t f, int sourceLevel, int flag )
{
   return guarded( [&] { P1toP1LinearRestriction().restrict( F( f ), (uint_t) sourceLevel, DoFType( flag ) ); } );
}
HYTEG_HOST_API int hyteg_host_prolongate( hh_function_t f, int sourceLevel, int flag )
{
   return guarded( [&] { P1toP1LinearProlongation().prolongate( F( f ), (uint_t) sourceLevel, DoFType( flag ) ); } );
}
HYTEG_HOST_API int hyteg_host_prolongate_and_add( hh_function_t f, int sourceLevel, int flag )
{
   return guarded( [&] { P1toP1LinearProlongation().prolongateAndAdd( F( f ), (uint_t) sourceLevel, DoFType( flag ) ); } );
}
HYTEG_HOST_API int hyteg_host_p1_to_p2( hh_function_t p1, hh_p2function_t p2, int p2Level, int flag )
{
   return guarded( [&] { P1toP2Conversion( F( p1 ), F2( p2 ), (uint_t) p2Level, DoFType( flag ) ); } );
}
HYTEG_HOST_API int hyteg_host_p2_to_p1( hh_p2function_t p2, hh_function_t p1, int p1Level, int flag )
{
   return guarded( [&] { P2toP1Conversion( F2( p2 ), F( p1 ), (uint_t) p1Level, DoFType( flag ) ); } );
}
HYTEG_HOST_API int hyteg_host_quadratic_prolongation_create( hh_storage_t s, int p1MinLevel, int p1MaxLevel, hh_quadratic_prolongation_t* out )
{
   return guarded( [&] {
      if ( p1MinLevel < 0 || p1MaxLevel < 0 )
         throw std::runtime_error( "quadratic_prolongation_create: negative level" );
      *out = new QuadraticProlongationH{ std::make_shared< P1toP1QuadraticProlongationThroughP2Injection >( SP( s ), (uint_t) p1MinLevel, (uint_t) p1MaxLevel ) };
   } );
}
HYTEG_HOST_API int hyteg_host_quadratic_prolongation_prolongate( hh_quadratic_prolongation_t p, hh_function_t f, int sourceLevel, int flag )
{
   return guarded( [&] { static_cast< QuadraticProlongationH* >( p )->p->prolongate( F( f ), (uint_t) sourceLevel, DoFType( flag ) ); } );
}
HYTEG_HOST_API int hyteg_host_quadratic_prolongation_destroy( hh_quadratic_prolongation_t p )
{
   return guarded( [&] { delete static_cast< QuadraticProlongationH* >( p ); } );
}
HYTEG_HOST_API int hyteg_host_fmg_create( hh_storage_t s, hh_solver_t gmg, int minL, int maxL, const unsigned* cyclesPerLevel, int nCycles, int prolongation,
                                          hh_level_callback_t postCycle, void* postCycleUser, hh_level_callback_t postProlongate,
                                          void* postProlongateUser, hh_solver_t* out )
{
   return guarded( [&] {
      using Op  = P1ConstantLaplaceOperator;
      auto g    = std::dynamic_pointer_cast< GeometricMultigridSolver< Op > >( static_cast< SolverH* >( gmg )->p );
      if ( !g )
         throw std::runtime_error( "fmg_create: not a geometric multigrid solver" );
      const auto cycles = fmgCycles( "fmg_create", minL, maxL, cyclesPerLevel, nCycles );
      const auto cbCycle = levelCallback( postCycle, postCycleUser ), cbProlongate = levelCallback( postProlongate, postProlongateUser );
      if ( prolongation == 0 )
         *out = new SolverH{ std::make_shared< FullMultigridSolver< Op > >( SP( s ), g, std::make_shared< P1toP1LinearProlongation >(), (uint_t) minL,
                                                                             (uint_t) maxL, cycles, cbCycle, cbProlongate ) };
      else if ( prolongation == 1 )
      {
         using Quadratic = P1toP1QuadraticProlongationThroughP2Injection;
         // the prolongation is used from minL to maxL - 1: its temporary spans the P2 levels minL - 1 .. maxL - 1
         auto p = std::make_shared< Quadratic >( SP( s ), (uint_t) minL, (uint_t) maxL );
         *out   = new SolverH{ std::make_shared< FullMultigridSolver< Op, GeometricMultigridSolver< Op >, Quadratic > >( SP( s ), g, p, (uint_t) minL, (uint_t) maxL,
                                                                                                                         cycles, cbCycle, cbProlongate ) };
      }
      else
         throw std::runtime_error( "fmg_create: prolongation must be 0 (linear) or 1 (quadratic)" );
   } );
}

HYTEG_HOST_API int hyteg_host_gmg_create( hh_storage_t s, int minL, int maxL, int smoother, double relax, int pre, int post, int wcycle,
                                          int cgMaxIter, double cgTol, hh_solver_t* out )
{
   return guarded( [&] {
      using Op = P1ConstantLaplaceOperator;
      auto sm  = scalarSmoother< Op >( smoother, SP( s ), minL, maxL, relax );
      if ( !sm ) // every other code: SOR
         sm = std::make_shared< SORSmoother< Op > >( relax );
      *out = new SolverH{ makeGmg< Op >( SP( s ), sm, cgCoarse< Op >( SP( s ), minL, cgMaxIter, cgTol ), minL, maxL, pre, post, 0, cycleOf( wcycle ) ) };
   } );
}
HYTEG_HOST_API int hyteg_host_gmg_set_use_graphs( hh_solver_t solver, int on )
{
   return guarded( [&] {
      auto g = std::dynamic_pointer_cast< GeometricMultigridSolver< P1ConstantLaplaceOperator > >( static_cast< SolverH* >( solver )->p );
      if ( !g )
         throw std::runtime_error( "gmg_set_use_graphs: not a geometric multigrid solver" );
      g->setUseGraphs( on != 0 );
   } );
}
HYTEG_HOST_API int hyteg_host_cg_set_use_device_scalars( hh_solver_t solver, int on )
{
   return guarded( [&] {
      using Op = P1ConstantLaplaceOperator;
      auto sp  = static_cast< SolverH* >( solver )->p;
      if ( auto g = std::dynamic_pointer_cast< GeometricMultigridSolver< Op > >( sp ) )
         sp = g->getCoarseSolver();
      auto cg = std::dynamic_pointer_cast< CGSolver< Op > >( sp );
      if ( !cg )
         throw std::runtime_error( "cg_set_use_device_scalars: neither a CG solver nor a multigrid solver with a CG coarse solver" );
      cg->setUseDeviceScalars( ( on & 1 ) != 0 );
      cg->setUseSingleLaunch( ( on & 2 ) != 0 );
   } );
}
HYTEG_HOST_API int hyteg_host_cg_iterations( hh_solver_t solver, int* iterations )
{
   return guarded( [&] { cgIterations< P1ConstantLaplaceOperator, SolverH >( "cg_iterations", solver, iterations ); } );
}
HYTEG_HOST_API int hyteg_host_gmg_replayed_cycles( hh_solver_t solver, int* count )
{
   return guarded( [&] {
      auto g = std::dynamic_pointer_cast< GeometricMultigridSolver< P1ConstantLaplaceOperator > >( static_cast< SolverH* >( solver )->p );
      if ( !g )
         throw std::runtime_error( "gmg_replayed_cycles: not a geometric multigrid solver" );
      *count = (int) g->replayedCycles();
   } );
}
HYTEG_HOST_API int hyteg_host_cg_create( hh_storage_t s, int minL, int maxL, int maxIter, double tol, hh_solver_t* out )
{
   return guarded( [&] {
      *out = new SolverH{ std::make_shared< CGSolver< P1ConstantLaplaceOperator > >( SP( s ), (uint_t) minL, (uint_t) maxL, (uint_t) maxIter, tol, tol ) };
   } );
}
HYTEG_HOST_API int hyteg_host_cg_create_preconditioned( hh_storage_t s, int minL, int maxL, int maxIter, double tol, hh_solver_t preconditioner,
                                                        hh_solver_t* out )
{
   return guarded( [&] {
      cgCreatePreconditioned< P1ConstantLaplaceOperator, SolverH >( "cg_create_preconditioned", s, minL, maxL, maxIter, tol, preconditioner, out );
   } );
}
HYTEG_HOST_API int hyteg_host_cg_set_use_fused_update( hh_solver_t solver, int on )
{
   return guarded( [&] {
      auto cg = std::dynamic_pointer_cast< CGSolver< P1ConstantLaplaceOperator > >( static_cast< SolverH* >( solver )->p );
      if ( !cg )
         throw std::runtime_error( "cg_set_use_fused_update: not a CG solver" );
      cg->setUseFusedUpdate( on != 0 );
   } );
}
HYTEG_HOST_API int hyteg_host_smoother_create( hh_storage_t s, int minL, int maxL, int smoother, double relax, hh_solver_t* out )
{
   return guarded( [&] { smootherCreate< P1ConstantLaplaceOperator, SolverH >( "smoother_create", s, minL, maxL, smoother, relax, out ); } );
}
/* ---- ChebyshevSmoother (src/hyteg/solvers/ChebyshevSmoother.hpp) ---- */
HYTEG_HOST_API int hyteg_host_chebyshev_coefficients( int order, double lower, double upper, double* out )
{
   return guarded( [&] {
      if ( order < 1 || !out )
         throw std::runtime_error( "chebyshev_coefficients: order >= 1 and an output array are needed" );
      const auto c = chebyshev::coefficients( (uint_t) order, lower, upper );
      std::copy( c.begin(), c.end(), out );
   } );
}
HYTEG_HOST_API int hyteg_host_chebyshev_estimate_radius( hh_operator_t op, int level, int maxIter, hh_function_t x, hh_function_t tmp, double* radius )
{
   return guarded( [&] {
      withOp( op, [&]( auto& A ) { *radius = chebyshev::estimateRadius( A, (uint_t) level, (uint_t) maxIter, A.getStorage(), F( x ), F( tmp ) ); } );
   } );
}
HYTEG_HOST_API int hyteg_host_chebyshev_create( hh_storage_t s, int minL, int maxL, int order, const double* radii, int nRadii, double upper,
                                                double lower, hh_solver_t* out )
{
   return guarded( [&] { *out = new SolverH{ makeChebyshev< P1ConstantLaplaceOperator >( s, minL, maxL, order, radii, nRadii, upper, lower ) }; } );
}
HYTEG_HOST_API int hyteg_host_chebyshev_set_fused( hh_solver_t solver, int on )
{
   return guarded( [&] {
      using Op = P1ConstantLaplaceOperator;
      auto sp  = static_cast< SolverH* >( solver )->p;
      if ( auto g = std::dynamic_pointer_cast< GeometricMultigridSolver< Op > >( sp ) )
         sp = g->getSmoother();
      auto ch = std::dynamic_pointer_cast< ChebyshevSmoother< Op > >( sp );
      if ( !ch )
         throw std::runtime_error( "chebyshev_set_fused: neither a Chebyshev smoother nor a multigrid solver that smooths with one" );
      ch->setFused( on != 0 );
   } );
}
HYTEG_HOST_API int hyteg_host_gmg_create_chebyshev( hh_storage_t s, int minL, int maxL, int order, const double* radii, int nRadii, double upper,
                                                    double lower, int pre, int post, int wcycle, int cgMaxIter, double cgTol, hh_solver_t* out )
{
   return guarded( [&] {
      using Op = P1ConstantLaplaceOperator;
      auto sm  = makeChebyshev< Op >( s, minL, maxL, order, radii, nRadii, upper, lower );
      *out = new SolverH{ makeGmg< Op >( SP( s ), sm, cgCoarse< Op >( SP( s ), minL, cgMaxIter, cgTol ), minL, maxL, pre, post, 0, cycleOf( wcycle ) ) };
   } );
}
HYTEG_HOST_API int hyteg_host_mixed_precision_jacobi_create( hh_storage_t s, int minL, int maxL, double relax, int fp32_sweeps, hh_solver_t* out )
{
   return guarded( [&] {
      if ( fp32_sweeps < 0 )
         throw std::runtime_error( "mixed_precision_jacobi_create: negative number of float sweeps" );
      *out = new SolverH{ std::make_shared< MixedPrecisionJacobiSmoother< P1ConstantLaplaceOperator > >( SP( s ), (uint_t) minL, (uint_t) maxL, relax,
                                                                                                         (uint_t) fp32_sweeps ) };
   } );
}
HYTEG_HOST_API int hyteg_host_solver_solve_steps( hh_solver_t solver, hh_operator_t laplace, hh_function_t x, hh_function_t b, int level, int steps )
{
   return guarded( [&] {
      auto* h = static_cast< OperatorH* >( laplace );
      if ( h->op.index() != 0 )
         throw std::runtime_error( "solver_solve_steps: the solvers are instantiated for the Laplace operator" );
      if ( steps < 0 )
         throw std::runtime_error( "solver_solve_steps: negative number of steps" );
      static_cast< SolverH* >( solver )->p->solveSteps( *std::get< 0 >( h->op ), F( x ), F( b ), (uint_t) level, (uint_t) steps );
   } );
}
HYTEG_HOST_API int hyteg_host_solver_solve( hh_solver_t solver, hh_operator_t laplace, hh_function_t x, hh_function_t b, int level )
{
   return guarded( [&] {
      auto* h = static_cast< OperatorH* >( laplace );
      if ( h->op.index() != 0 )
         throw std::runtime_error( "solver_solve: the solvers are instantiated for the Laplace operator" );
      static_cast< SolverH* >( solver )->p->solve( *std::get< 0 >( h->op ), F( x ), F( b ), (uint_t) level );
   } );
}
HYTEG_HOST_API int hyteg_host_solver_destroy( hh_solver_t solver )
{
   return guarded( [&] { delete static_cast< SolverH* >( solver ); } );
}

/* ---- P1-P1 Stokes (src/mixed_operator/P1P1StokesOperator.hpp, src/hyteg/solvers/UzawaSmoother.hpp) ---- */
HYTEG_HOST_API int hyteg_host_stokes_function_create( hh_storage_t s, const char* name, int minL, int maxL, hh_stokes_function_t* out )
{
   return P1P1::functionCreate( s, name, minL, maxL, out );
}
HYTEG_HOST_API int hyteg_host_stokes_function_destroy( hh_stokes_function_t f ) { return P1P1::destroy< P1P1::FunctionHandle >( f ); }
HYTEG_HOST_API int hyteg_host_stokes_function_component( hh_stokes_function_t f, int k, hh_function_t* out )
{
   return guarded( [&] {
      if ( k < 0 || k > 3 )
         throw std::runtime_error( "stokes_function_component: k = 0, 1, 2 (velocity) or 3 (pressure)" );
      *out = k < 3 ? P1P1::velocityView( f, k ) : P1P1::pressureView( f );
   } );
}
HYTEG_HOST_API int hyteg_host_stokes_function_assign( hh_stokes_function_t dst, int n, const double* scalars, const hh_stokes_function_t* fs, int level, int flag )
{
   return P1P1::functionAssign( dst, n, scalars, fs, level, flag );
}
HYTEG_HOST_API int hyteg_host_stokes_function_dot( hh_stokes_function_t a, hh_stokes_function_t b, int level, int flag, double* out )
{
   return P1P1::functionDot( a, b, level, flag, out );
}
HYTEG_HOST_API int hyteg_host_project_mean( hh_function_t pressure, int level )
{
   return guarded( [&] { projectMean( F( pressure ), (uint_t) level ); } );
}
HYTEG_HOST_API int hyteg_host_stokes_operator_create( hh_storage_t s, int minL, int maxL, hh_stokes_operator_t* out )
{
   return P1P1::operatorCreate( s, minL, maxL, out );
}
HYTEG_HOST_API int hyteg_host_stokes_operator_destroy( hh_stokes_operator_t op ) { return P1P1::destroy< P1P1::OperatorHandle >( op ); }
HYTEG_HOST_API int hyteg_host_stokes_operator_apply( hh_stokes_operator_t op, hh_stokes_function_t src, hh_stokes_function_t dst, int level, int flag )
{
   return P1P1::operatorApply( op, src, dst, level, flag );
}
HYTEG_HOST_API int hyteg_host_stokes_uzawa_create( hh_storage_t s, int minL, int maxL, double relax, int velocity_iterations, int velocity_smoother,
                                                   double velocity_relax, hh_stokes_solver_t* out )
{
   return guarded( [&] {
      using Op     = P1P1StokesOperator;
      auto storage = SP( s );
      auto scalar  = scalarSmoother< P1ConstantLaplaceOperator >( velocity_smoother, storage, minL, maxL, velocity_relax );
      if ( !scalar )
         throw std::runtime_error( "stokes_uzawa_create: unknown velocity smoother" );
      auto velocity = std::make_shared< StokesVelocityBlockBlockDiagonalPreconditioner< Op > >( storage, scalar );
      *out          = new P1P1::SolverHandle{ std::make_shared< UzawaSmoother< Op > >( storage, velocity, (uint_t) minL, (uint_t) maxL, relax,
                                                                                       Inner | NeumannBoundary | FreeslipBoundary,
                                                                                       (uint_t) velocity_iterations ) };
   } );
}
// coarse: 0 = dense LU on the host (stand-in for PETScLUSolver, single rank), 1 = MinResSolver preconditioned with
// StokesPressureBlockPreconditioner< P1P1StokesOperator, P1LumpedInvMassOperator > as apps/stokesSphere/StokesSphere.cpp:227-237
// composes it (any number of ranks)
HYTEG_HOST_API int hyteg_host_stokes_gmg_create_with_coarse( hh_storage_t s, hh_stokes_solver_t smoother, int minL, int maxL, int pre, int post,
                                                             int increment, int project_mean_after_restriction, int coarse, int coarse_max_iter,
                                                             double coarse_rel_tol, hh_stokes_solver_t* out )
{
   return guarded( [&] {
      using Op     = P1P1StokesOperator;
      auto storage = SP( s );
      std::shared_ptr< Solver< Op > > coarseSolver;
      if ( coarse == 0 )
         coarseSolver = std::make_shared< DenseCoarseGridSolver< Op > >( storage, (uint_t) minL );
      else if ( coarse == 1 )
         coarseSolver = P1P1::pressureMinres( storage, minL, minL, coarse_max_iter, coarse_rel_tol );
      else
         throw std::runtime_error( "stokes_gmg_create: unknown coarse-grid solver" );
      *out = new P1P1::SolverHandle{ makeGmg< Op, P1P1StokesToP1P1StokesRestriction, P1P1StokesToP1P1StokesProlongation >(
          storage, static_cast< P1P1::SolverHandle* >( smoother )->p, coarseSolver, minL, maxL, pre, post, increment, CycleType::VCYCLE,
          project_mean_after_restriction != 0 ) };
   } );
}
HYTEG_HOST_API int hyteg_host_stokes_gmg_create( hh_storage_t s, hh_stokes_solver_t smoother, int minL, int maxL, int pre, int post, int increment,
                                                 int project_mean_after_restriction, hh_stokes_solver_t* out )
{
   return hyteg_host_stokes_gmg_create_with_coarse( s, smoother, minL, maxL, pre, post, increment, project_mean_after_restriction, 0, 0, 0.0, out );
}
// MinResSolver< P1P1StokesOperator > on its own: preconditioner 0 identity, 1 pressure block (lumped inverse mass),
// 2 StokesBlockDiagonalPreconditioner with `velocity_steps` V(2,2) cycles of the scalar Laplace operator per velocity component
// (apps/stokesSphere/StokesSphere.cpp:198-222, tests/hyteg/convergence/P1Stokes3DMinResConvergenceTest.cpp:166-183)
HYTEG_HOST_API int hyteg_host_stokes_minres_create( hh_storage_t s, int minL, int maxL, int max_iter, double rel_tol, int preconditioner,
                                                    int velocity_steps, hh_stokes_solver_t* out )
{
   return guarded( [&] {
      using Op     = P1P1StokesOperator;
      auto storage = SP( s );
      std::shared_ptr< Solver< Op > > prec;
      if ( preconditioner == 0 )
         prec = std::make_shared< IdentityPreconditioner< Op > >();
      else if ( preconditioner == 1 )
         prec = std::make_shared< StokesPressureBlockPreconditioner< Op, P1LumpedInvMassOperator > >( storage, (uint_t) minL, (uint_t) maxL );
      else if ( preconditioner == 2 )
      {
         using L       = P1ConstantLaplaceOperator;
         auto smoother = std::make_shared< GaussSeidelSmoother< L > >();
         auto coarse   = std::make_shared< CGSolver< L > >( storage, (uint_t) minL, (uint_t) maxL );
         auto gmg      = makeGmg< L >( storage, smoother, coarse, minL, maxL, 2, 2, 0, CycleType::VCYCLE );
         prec = std::make_shared< StokesBlockDiagonalPreconditioner< Op, P1LumpedInvMassOperator > >( storage, (uint_t) minL, (uint_t) maxL,
                                                                                                       (uint_t) velocity_steps, gmg );
      }
      else
         throw std::runtime_error( "stokes_minres_create: unknown preconditioner" );
      auto solver = std::make_shared< MinResSolver< Op > >( storage, (uint_t) minL, (uint_t) maxL, (uint_t) max_iter, rel_tol, 1e-16, prec );
      *out        = new P1P1::SolverHandle{ solver };
   } );
}
HYTEG_HOST_API int hyteg_host_stokes_minres_iterations( hh_stokes_solver_t solver, int* iterations )
{
   return guarded( [&] {
      auto* m = dynamic_cast< MinResSolver< P1P1StokesOperator >* >( &P1P1::solver( solver ) );
      if ( !m )
         throw std::runtime_error( "stokes_minres_iterations: not a MinResSolver" );
      *iterations = (int) m->getIterations();
   } );
}
/* ---- strong free-slip (P1ProjectNormalOperator.hpp, composites/StrongFreeSlipWrapper.hpp) ---- */
HYTEG_HOST_API int hyteg_host_storage_shell_size( int level, int* out )
{
   return guarded( [&] {
      *out = hyteg_hip_p1_shell_size( level );
      if ( *out == 0 )
         throw std::runtime_error( "storage_shell_size: level out of range" );
   } );
}
HYTEG_HOST_API int hyteg_host_storage_shell_points( hh_storage_t s, int li, int level, double* xyz )
{
   return guarded( [&] {
      const auto pts = freeslip::shellPoints( S( s ), S( s ).getLocalCell( (uint_t) li ), (uint_t) level );
      for ( size_t q = 0; q < pts.size(); ++q )
         for ( size_t r = 0; r < 3; ++r )
            xyz[3 * q + r] = pts[q][r];
   } );
}
HYTEG_HOST_API int hyteg_host_project_normal_create( hh_storage_t s, int minL, int maxL, hh_normal_callback_t normal, void* user,
                                                     hh_project_normal_t* out )
{
   return P1FreeSlip::projectionCreate( s, minL, maxL, normal, user, out );
}
HYTEG_HOST_API int hyteg_host_project_normal_destroy( hh_project_normal_t p )
{
   return guarded( [&] { delete static_cast< P1FreeSlip::ProjectionHandle* >( p ); } );
}
HYTEG_HOST_API int hyteg_host_project_normal_project( hh_project_normal_t p, hh_function_t u, hh_function_t v, hh_function_t w, int level, int flag )
{
   return guarded( [&] { P1FreeSlip::projection( p ).project( F( u ), F( v ), F( w ), (uint_t) level, DoFType( flag ) ); } );
}
HYTEG_HOST_API int hyteg_host_project_normal_project_stokes( hh_project_normal_t p, hh_stokes_function_t f, int level, int flag )
{
   return guarded( [&] { P1FreeSlip::projection( p ).project( P1P1::fn( f ), (uint_t) level, DoFType( flag ) ); } );
}
HYTEG_HOST_API int hyteg_host_stokes_freeslip_wrapper_create( hh_stokes_operator_t op, hh_project_normal_t p, int flag, int pre_projection,
                                                              hh_freeslip_wrapper_t* out )
{
   return P1FreeSlip::wrapperCreate( op, p, flag, pre_projection, out );
}
HYTEG_HOST_API int hyteg_host_stokes_freeslip_wrapper_destroy( hh_freeslip_wrapper_t w )
{
   return guarded( [&] { delete static_cast< P1FreeSlip::WrapperHandle* >( w ); } );
}
HYTEG_HOST_API int hyteg_host_stokes_freeslip_wrapper_apply( hh_freeslip_wrapper_t w, hh_stokes_function_t src, hh_stokes_function_t dst, int level,
                                                             int flag )
{
   return P1FreeSlip::wrapperApply( w, src, dst, level, flag );
}
HYTEG_HOST_API int hyteg_host_stokes_freeslip_minres_create( hh_storage_t s, int minL, int maxL, int max_iter, double rel_tol, int preconditioner,
                                                             int pre_projection, hh_freeslip_solver_t* out )
{
   return P1FreeSlip::minresCreate( s, minL, maxL, max_iter, rel_tol, preconditioner, pre_projection, out );
}
HYTEG_HOST_API int hyteg_host_stokes_freeslip_minres_solve( hh_freeslip_solver_t solver, hh_freeslip_wrapper_t w, hh_stokes_function_t x,
                                                            hh_stokes_function_t b, int level )
{
   return P1FreeSlip::solve( solver, w, x, b, level );
}
HYTEG_HOST_API int hyteg_host_stokes_freeslip_minres_iterations( hh_freeslip_solver_t solver, int* iterations )
{
   return P1FreeSlip::iterations( solver, iterations );
}
HYTEG_HOST_API int hyteg_host_stokes_freeslip_minres_destroy( hh_freeslip_solver_t solver )
{
   return guarded( [&] { delete static_cast< P1FreeSlip::SolverHandle* >( solver ); } );
}
/* the same for P2 velocities (P2ProjectNormalOperator.hpp) and the Taylor-Hood operator */
HYTEG_HOST_API int hyteg_host_storage_edge_shell_size( int level, int* out )
{
   return guarded( [&] {
      *out = hyteg_hip_p2_edge_shell_size( level );
      if ( *out == 0 )
         throw std::runtime_error( "storage_edge_shell_size: level out of range" );
   } );
}
HYTEG_HOST_API int hyteg_host_storage_edge_shell_points( hh_storage_t s, int li, int level, double* xyz )
{
   return guarded( [&] {
      const auto pts = freeslip::edgeShellPoints( S( s ), S( s ).getLocalCell( (uint_t) li ), (uint_t) level );
      for ( size_t q = 0; q < pts.size(); ++q )
         for ( size_t r = 0; r < 3; ++r )
            xyz[3 * q + r] = pts[q][r];
   } );
}
HYTEG_HOST_API int hyteg_host_p2_project_normal_create( hh_storage_t s, int minL, int maxL, hh_normal_callback_t normal, void* user,
                                                        hh_p2_project_normal_t* out )
{
   return THFreeSlip::projectionCreate( s, minL, maxL, normal, user, out );
}
HYTEG_HOST_API int hyteg_host_p2_project_normal_destroy( hh_p2_project_normal_t p )
{
   return guarded( [&] { delete static_cast< THFreeSlip::ProjectionHandle* >( p ); } );
}
HYTEG_HOST_API int hyteg_host_p2_project_normal_project( hh_p2_project_normal_t p, hh_p2function_t u, hh_p2function_t v, hh_p2function_t w, int level,
                                                         int flag )
{
   return guarded( [&] { THFreeSlip::projection( p ).project( F2( u ), F2( v ), F2( w ), (uint_t) level, DoFType( flag ) ); } );
}
HYTEG_HOST_API int hyteg_host_p2_project_normal_project_stokes( hh_p2_project_normal_t p, hh_th_function_t f, int level, int flag )
{
   return guarded( [&] { THFreeSlip::projection( p ).project( TH::fn( f ), (uint_t) level, DoFType( flag ) ); } );
}
HYTEG_HOST_API int hyteg_host_th_freeslip_wrapper_create( hh_th_operator_t op, hh_p2_project_normal_t p, int flag, int pre_projection,
                                                          hh_freeslip_wrapper_t* out )
{
   return THFreeSlip::wrapperCreate( op, p, flag, pre_projection, out );
}
HYTEG_HOST_API int hyteg_host_th_freeslip_wrapper_destroy( hh_freeslip_wrapper_t w )
{
   return guarded( [&] { delete static_cast< THFreeSlip::WrapperHandle* >( w ); } );
}
HYTEG_HOST_API int hyteg_host_th_freeslip_wrapper_apply( hh_freeslip_wrapper_t w, hh_th_function_t src, hh_th_function_t dst, int level, int flag )
{
   return THFreeSlip::wrapperApply( w, src, dst, level, flag );
}
HYTEG_HOST_API int hyteg_host_th_freeslip_minres_create( hh_storage_t s, int minL, int maxL, int max_iter, double rel_tol, int preconditioner,
                                                         int pre_projection, hh_freeslip_solver_t* out )
{
   return THFreeSlip::minresCreate( s, minL, maxL, max_iter, rel_tol, preconditioner, pre_projection, out );
}
HYTEG_HOST_API int hyteg_host_th_freeslip_minres_solve( hh_freeslip_solver_t solver, hh_freeslip_wrapper_t w, hh_th_function_t x, hh_th_function_t b,
                                                        int level )
{
   return THFreeSlip::solve( solver, w, x, b, level );
}
HYTEG_HOST_API int hyteg_host_th_freeslip_minres_iterations( hh_freeslip_solver_t solver, int* iterations )
{
   return THFreeSlip::iterations( solver, iterations );
}
HYTEG_HOST_API int hyteg_host_th_freeslip_minres_destroy( hh_freeslip_solver_t solver )
{
   return guarded( [&] { delete static_cast< THFreeSlip::SolverHandle* >( solver ); } );
}
// MinResSolver< P1ConstantLaplaceOperator > with JacobiPreconditioner( jacobi_iterations ) (0: identity), as
// tests/hyteg/convergence/P1MinResConvergenceTest.cpp:68-72
HYTEG_HOST_API int hyteg_host_solver_create_minres( hh_storage_t s, int minL, int maxL, int max_iter, double rel_tol, int jacobi_iterations, hh_solver_t* out )
{
   return guarded( [&] {
      using L      = P1ConstantLaplaceOperator;
      auto storage = SP( s );
      std::shared_ptr< Solver< L > > prec;
      if ( jacobi_iterations > 0 )
         prec = std::make_shared< JacobiPreconditioner< L > >( storage, (uint_t) minL, (uint_t) maxL, (uint_t) jacobi_iterations );
      else
         prec = std::make_shared< IdentityPreconditioner< L > >();
      *out = new SolverH{ std::make_shared< MinResSolver< L > >( storage, (uint_t) minL, (uint_t) maxL, (uint_t) max_iter, rel_tol, 1e-16, prec ) };
   } );
}
HYTEG_HOST_API int hyteg_host_stokes_solver_solve( hh_stokes_solver_t solver, hh_stokes_operator_t op, hh_stokes_function_t x, hh_stokes_function_t b, int level )
{
   return P1P1::solverSolve( solver, op, x, b, level );
}
HYTEG_HOST_API int hyteg_host_stokes_solver_destroy( hh_stokes_solver_t solver ) { return P1P1::destroy< P1P1::SolverHandle >( solver ); }

// ---- variable-viscosity Stokes: P1ElementwiseAffineEpsilonOperator, P1P1ElementwiseAffineEpsilonStokesOperator, MinResSolver ----
using Epsilon       = P1ElementwiseAffineEpsilonOperator;
using EpsilonStokes = P1P1ElementwiseAffineEpsilonStokesOperator;
struct EpsilonH
{
   std::shared_ptr< P1Function< double > > mu; // the operator holds a reference: the handle keeps the function alive
   std::shared_ptr< Epsilon >              p;
   FunctionH                               invDiag[3]; // borrowed views
};
struct EpsilonStokesH
{
   std::shared_ptr< P1Function< double > > mu;
   std::shared_ptr< EpsilonStokes >        p;
};
struct EpsilonSolverH
{
   std::shared_ptr< Solver< Epsilon > > p;
};
struct EpsilonStokesSolverH
{
   std::shared_ptr< P1Function< double > >        mu; // of the viscosity-weighted preconditioner, or null
   std::shared_ptr< Solver< EpsilonStokes > >     preconditioner;
   std::shared_ptr< MinResSolver< EpsilonStokes > > p;
   bool                                           smoothsVelocity = false; // its preconditioner reads the velocity operator's inverse diagonals
   // assembled on first use: the Stokes operator does not assemble them itself (the pressure preconditioners never read them)
   void prepare( EpsilonStokes& op ) const
   {
      if ( smoothsVelocity && !op.viscOp.hasInverseDiagonalValues() )
         op.viscOp.computeInverseDiagonalOperatorValues();
   }
};
static Epsilon& EP( hh_epsilon_t op )
{
   if ( !op )
      throw std::runtime_error( "null epsilon operator" );
   return *static_cast< EpsilonH* >( op )->p;
}
static EpsilonStokes& EPS( hh_epsilon_stokes_t op )
{
   if ( !op )
      throw std::runtime_error( "null epsilon Stokes operator" );
   return *static_cast< EpsilonStokesH* >( op )->p;
}
// three function handles as one P1VectorFunction (a view: the handles keep the components)
static P1VectorFunction< double > vectorOf( const hh_function_t* f )
{
   if ( !f || !f[0] || !f[1] || !f[2] )
      throw std::runtime_error( "epsilon: three component functions" );
   return P1VectorFunction< double >( { static_cast< FunctionH* >( f[0] )->p, static_cast< FunctionH* >( f[1] )->p, static_cast< FunctionH* >( f[2] )->p } );
}
static std::shared_ptr< P1Function< double > > viscosityOf( const char* who, hh_function_t mu, int minL, int maxL )
{
   if ( !mu || minL < 0 || maxL < minL )
      throw std::runtime_error( std::string( who ) + ": needs a viscosity function and 0 <= min_level <= max_level" );
   return static_cast< FunctionH* >( mu )->p;
}
HYTEG_HOST_API int hyteg_host_epsilon_create( hh_storage_t s, int minL, int maxL, hh_function_t mu, hh_epsilon_t* out )
{
   return guarded( [&] {
      auto h = std::make_unique< EpsilonH >();
      h->mu  = viscosityOf( "epsilon_create", mu, minL, maxL );
      h->p   = std::make_shared< Epsilon >( SP( s ), (uint_t) minL, (uint_t) maxL, *h->mu );
      *out   = h.release();
   } );
}
HYTEG_HOST_API int hyteg_host_epsilon_destroy( hh_epsilon_t op )
{
   return guarded( [&] { delete static_cast< EpsilonH* >( op ); } );
}
HYTEG_HOST_API int hyteg_host_epsilon_apply( hh_epsilon_t op, const hh_function_t* src, const hh_function_t* dst, int level, int flag, int update )
{
   return guarded( [&] { EP( op ).apply( vectorOf( src ), vectorOf( dst ), (uint_t) level, DoFType( flag ), update ? Add : Replace ); } );
}
HYTEG_HOST_API int hyteg_host_epsilon_compute_inverse_diagonal( hh_epsilon_t op )
{
   return guarded( [&] { EP( op ).computeInverseDiagonalOperatorValues(); } );
}
HYTEG_HOST_API int hyteg_host_epsilon_inverse_diagonal( hh_epsilon_t op, hh_function_t* out )
{
   return guarded( [&] {
      auto*      h = static_cast< EpsilonH* >( op );
      const auto d = EP( op ).getInverseDiagonalValues();
      for ( int k = 0; k < 3; ++k )
      {
         h->invDiag[k].p = viewOf( d, ( *d )[(uint_t) k] );
         out[k]          = &h->invDiag[k];
      }
   } );
}
HYTEG_HOST_API int hyteg_host_epsilon_smooth_jac( hh_epsilon_t op, const hh_function_t* dst, const hh_function_t* rhs, const hh_function_t* src,
                                                  double relax, int level, int flag )
{
   return guarded( [&] { EP( op ).smooth_jac( vectorOf( dst ), vectorOf( rhs ), vectorOf( src ), relax, (uint_t) level, DoFType( flag ) ); } );
}
HYTEG_HOST_API int hyteg_host_epsilon_set_fused( hh_epsilon_t op, int on )
{
   return guarded( [&] { EP( op ).setFused( on != 0 ); } );
}
HYTEG_HOST_API int hyteg_host_epsilon_residual( hh_epsilon_t op, const hh_function_t* x, const hh_function_t* b, const hh_function_t* r, int level, int flag )
{
   return guarded( [&] { EP( op ).residual( vectorOf( x ), vectorOf( b ), vectorOf( r ), (uint_t) level, DoFType( flag ) ); } );
}

// ---- the solvers instantiated for the epsilon operator, acting on three component functions ----
// a multigrid cycle on P1 vector functions: the linear P1 transfer on every component, CG on the coarsest level
static std::shared_ptr< Solver< Epsilon > > epsilonGmg( hh_storage_t s, std::shared_ptr< Solver< Epsilon > > smoother, int minL, int maxL, int pre, int post,
                                                        int wcycle, int cgMaxIter, double cgTol )
{
   return makeGmg< Epsilon, P1VectorFunctionLinearRestriction, P1VectorFunctionLinearProlongation >(
       SP( s ), smoother, cgCoarse< Epsilon >( SP( s ), minL, cgMaxIter, cgTol ), minL, maxL, pre, post, 0, cycleOf( wcycle ) );
}
// the operator has no Gauss-Seidel sweep: weighted Jacobi (0) and the identity (-1)
static std::shared_ptr< Solver< Epsilon > > epsilonSmoother( const char* who, hh_storage_t s, int minL, int maxL, int code, double relax )
{
   if ( code == 0 )
      return std::make_shared< WeightedJacobiSmoother< Epsilon > >( SP( s ), (uint_t) minL, (uint_t) maxL, relax );
   if ( code == -1 )
      return std::make_shared< IdentityPreconditioner< Epsilon > >();
   throw std::runtime_error( std::string( who ) + ": smoother 0 (weighted Jacobi) or -1 (identity); the epsilon operator has no SOR sweep" );
}
// chebyshev::estimateRadius from a start vector of incommensurate waves (components along every eigenvector)
static double epsilonRadius( const Epsilon& op, uint_t level, uint_t iterations )
{
   auto                       storage = op.getStorage();
   P1VectorFunction< double > x( "epsilon_radius_x", storage, level, level ), tmp( "epsilon_radius_tmp", storage, level, level );
   x.interpolate( { []( const Point3D& q ) { return std::sin( 7.3 * q[0] + 3.1 * q[1] + 1.7 * q[2] + 0.4 ); },
                    []( const Point3D& q ) { return std::cos( 2.9 * q[0] - 6.1 * q[1] + 4.3 * q[2] ); },
                    []( const Point3D& q ) { return std::sin( 5.3 * q[0] * q[1] - 3.7 * q[2] + 1.1 ); } },
                  level, All );
   return chebyshev::estimateRadius( op, level, iterations, storage, x, tmp );
}
HYTEG_HOST_API int hyteg_host_epsilon_chebyshev_estimate_radius( hh_epsilon_t op, int level, int maxIter, double* radius )
{
   return guarded( [&] { *radius = epsilonRadius( EP( op ), (uint_t) level, (uint_t) maxIter ); } );
}
HYTEG_HOST_API int hyteg_host_epsilon_cg_create( hh_storage_t s, int minL, int maxL, int maxIter, double tol, hh_epsilon_solver_t preconditioner,
                                                 hh_epsilon_solver_t* out )
{
   return guarded( [&] {
      if ( preconditioner )
         cgCreatePreconditioned< Epsilon, EpsilonSolverH >( "epsilon_cg_create", s, minL, maxL, maxIter, tol, preconditioner, out );
      else
         *out = new EpsilonSolverH{ std::make_shared< CGSolver< Epsilon > >( SP( s ), (uint_t) minL, (uint_t) maxL, (uint_t) maxIter, tol, tol ) };
   } );
}
HYTEG_HOST_API int hyteg_host_epsilon_cg_iterations( hh_epsilon_solver_t solver, int* iterations )
{
   return guarded( [&] { cgIterations< Epsilon, EpsilonSolverH >( "epsilon_cg_iterations", solver, iterations ); } );
}
HYTEG_HOST_API int hyteg_host_epsilon_smoother_create( hh_storage_t s, int minL, int maxL, int smoother, double relax, hh_epsilon_solver_t* out )
{
   return guarded( [&] { *out = new EpsilonSolverH{ epsilonSmoother( "epsilon_smoother_create", s, minL, maxL, smoother, relax ) }; } );
}
HYTEG_HOST_API int hyteg_host_epsilon_gmg_create( hh_storage_t s, int minL, int maxL, double relax, int pre, int post, int wcycle, int cgMaxIter,
                                                  double cgTol, hh_epsilon_solver_t* out )
{
   return guarded( [&] {
      *out = new EpsilonSolverH{ epsilonGmg( s, epsilonSmoother( "epsilon_gmg_create", s, minL, maxL, 0, relax ), minL, maxL, pre, post, wcycle, cgMaxIter,
                                             cgTol ) };
   } );
}
HYTEG_HOST_API int hyteg_host_epsilon_chebyshev_create( hh_storage_t s, int minL, int maxL, int order, const double* radii, int nRadii, double upper,
                                                        double lower, hh_epsilon_solver_t* out )
{
   return guarded( [&] { *out = new EpsilonSolverH{ makeChebyshev< Epsilon >( s, minL, maxL, order, radii, nRadii, upper, lower ) }; } );
}
HYTEG_HOST_API int hyteg_host_epsilon_gmg_create_chebyshev( hh_storage_t s, int minL, int maxL, int order, const double* radii, int nRadii, double upper,
                                                            double lower, int pre, int post, int wcycle, int cgMaxIter, double cgTol,
                                                            hh_epsilon_solver_t* out )
{
   return guarded( [&] {
      *out = new EpsilonSolverH{
          epsilonGmg( s, makeChebyshev< Epsilon >( s, minL, maxL, order, radii, nRadii, upper, lower ), minL, maxL, pre, post, wcycle, cgMaxIter, cgTol ) };
   } );
}
HYTEG_HOST_API int hyteg_host_epsilon_solver_solve( hh_epsilon_solver_t solver, hh_epsilon_t op, const hh_function_t* x, const hh_function_t* b, int level )
{
   return guarded( [&] {
      if ( !solver )
         throw std::runtime_error( "null epsilon solver" );
      static_cast< EpsilonSolverH* >( solver )->p->solve( EP( op ), vectorOf( x ), vectorOf( b ), (uint_t) level );
   } );
}
HYTEG_HOST_API int hyteg_host_epsilon_solver_destroy( hh_epsilon_solver_t solver )
{
   return guarded( [&] { delete static_cast< EpsilonSolverH* >( solver ); } );
}

HYTEG_HOST_API int hyteg_host_epsilon_stokes_create( hh_storage_t s, int minL, int maxL, hh_function_t mu, hh_epsilon_stokes_t* out )
{
   return guarded( [&] {
      auto h = std::make_unique< EpsilonStokesH >();
      h->mu  = viscosityOf( "epsilon_stokes_create", mu, minL, maxL );
      h->p   = std::make_shared< EpsilonStokes >( SP( s ), (uint_t) minL, (uint_t) maxL, *h->mu );
      *out   = h.release();
   } );
}
HYTEG_HOST_API int hyteg_host_epsilon_stokes_destroy( hh_epsilon_stokes_t op )
{
   return guarded( [&] { delete static_cast< EpsilonStokesH* >( op ); } );
}
HYTEG_HOST_API int hyteg_host_epsilon_stokes_apply( hh_epsilon_stokes_t op, hh_stokes_function_t src, hh_stokes_function_t dst, int level, int flag )
{
   return guarded( [&] { EPS( op ).apply( P1P1::fn( src ), P1P1::fn( dst ), (uint_t) level, DoFType( flag ) ); } );
}
// MinResSolver< P1P1ElementwiseAffineEpsilonStokesOperator >; preconditioner 0 identity, 1 StokesPressureBlockPreconditioner< .,
// P1LumpedInvMassOperator > (solvertemplates::stokesMinResSolver, StokesSolverTemplates.hpp:54-69), 2 the same weighted with mu
HYTEG_HOST_API int hyteg_host_epsilon_stokes_minres_create( hh_storage_t s, int minL, int maxL, int max_iter, double rel_tol, int preconditioner,
                                                            hh_function_t mu, hh_epsilon_stokes_solver_t* out )
{
   return guarded( [&] {
      auto storage = SP( s );
      auto h       = std::make_unique< EpsilonStokesSolverH >();
      if ( preconditioner == 0 )
         h->preconditioner = std::make_shared< IdentityPreconditioner< EpsilonStokes > >();
      else if ( preconditioner == 1 )
         h->preconditioner =
             std::make_shared< StokesPressureBlockPreconditioner< EpsilonStokes, P1LumpedInvMassOperator > >( storage, (uint_t) minL, (uint_t) maxL );
      else if ( preconditioner == 2 )
      {
         h->mu             = viscosityOf( "epsilon_stokes_minres_create (viscosity-weighted preconditioner)", mu, minL, maxL );
         h->preconditioner = std::make_shared< StokesViscosityWeightedPressureBlockPreconditioner< EpsilonStokes > >( storage, (uint_t) minL,
                                                                                                                     (uint_t) maxL, *h->mu );
      }
      else
         throw std::runtime_error( "epsilon_stokes_minres_create: unknown preconditioner" );
      h->p = std::make_shared< MinResSolver< EpsilonStokes > >( storage, (uint_t) minL, (uint_t) maxL, (uint_t) max_iter, rel_tol, 1e-16,
                                                                h->preconditioner );
      *out = h.release();
   } );
}
// MinResSolver preconditioned with StokesVectorBlockDiagonalPreconditioner: velocityCycles multigrid V-cycles on the epsilon operator
// (smoother 0 weighted Jacobi( relax ), 1 Chebyshev( order; radii: none = estimated per level here, one, or one per level ); pre = post
// steps, CG on the coarsest level) and the lumped inverse mass on the pressure, weighted with mu if viscosityWeighted.  mu: the
// viscosity of the operator the solver will be used with (the radii are estimated on an operator built from it).
HYTEG_HOST_API int hyteg_host_epsilon_stokes_minres_create_block( hh_storage_t s, int minL, int maxL, int max_iter, double rel_tol, int viscosityWeighted,
                                                                  hh_function_t mu, int velocityCycles, int smoother, int order, const double* radii,
                                                                  int nRadii, double relax, int pre, int post, int cgMaxIter, double cgTol,
                                                                  hh_epsilon_stokes_solver_t* out )
{
   return guarded( [&] {
      const char* who     = "epsilon_stokes_minres_create_block";
      auto        storage = SP( s );
      auto        h       = std::make_unique< EpsilonStokesSolverH >();
      // MINRES needs a symmetric positive definite preconditioner
      if ( smoother != 0 && smoother != 1 )
         throw std::runtime_error( std::string( who ) + ": smoother 0 (weighted Jacobi) or 1 (Chebyshev); an SOR sweep is not symmetric" );
      if ( pre != post || pre < 1 )
         throw std::runtime_error( std::string( who ) + ": a symmetric cycle needs pre = post >= 1 smoothing steps" );
      if ( velocityCycles < 1 )
         throw std::runtime_error( std::string( who ) + ": velocity_cycles >= 1" );
      h->mu = viscosityOf( who, mu, minL, maxL );
      std::shared_ptr< Solver< Epsilon > > sm;
      if ( smoother == 0 )
         sm = epsilonSmoother( who, s, minL, maxL, 0, relax );
      else
      {
         std::vector< double > rho( radii, radii + ( radii ? nRadii : 0 ) );
         if ( rho.empty() )
         {
            Epsilon probe( storage, (uint_t) minL, (uint_t) maxL, *h->mu );
            probe.computeInverseDiagonalOperatorValues();
            for ( int l = minL; l <= maxL; ++l )
               rho.push_back( epsilonRadius( probe, (uint_t) l, 20 ) );
         }
         sm = makeChebyshev< Epsilon >( s, minL, maxL, order, rho.data(), (int) rho.size(), 1.2, 0.3 );
      }
      auto velocity      = epsilonGmg( s, sm, minL, maxL, pre, post, 0, cgMaxIter, cgTol );
      h->smoothsVelocity = true;
      if ( viscosityWeighted )
         h->preconditioner = std::make_shared< StokesVectorBlockDiagonalPreconditioner< EpsilonStokes, Solver< Epsilon >, P1ViscosityWeightedLumpedInvMassOperator > >(
             velocity, std::make_shared< P1ViscosityWeightedLumpedInvMassOperator >( storage, (uint_t) minL, (uint_t) maxL, *h->mu ), (uint_t) velocityCycles );
      else
         h->preconditioner = std::make_shared< StokesVectorBlockDiagonalPreconditioner< EpsilonStokes, Solver< Epsilon >, P1LumpedInvMassOperator > >(
             velocity, std::make_shared< P1LumpedInvMassOperator >( storage, (uint_t) minL, (uint_t) maxL ), (uint_t) velocityCycles );
      h->p = std::make_shared< MinResSolver< EpsilonStokes > >( storage, (uint_t) minL, (uint_t) maxL, (uint_t) max_iter, rel_tol, 1e-16,
                                                                h->preconditioner );
      *out = h.release();
   } );
}
static EpsilonStokesSolverH& EPSS( hh_epsilon_stokes_solver_t solver )
{
   if ( !solver )
      throw std::runtime_error( "null epsilon Stokes solver" );
   return *static_cast< EpsilonStokesSolverH* >( solver );
}
HYTEG_HOST_API int hyteg_host_epsilon_stokes_minres_solve( hh_epsilon_stokes_solver_t solver, hh_epsilon_stokes_t op, hh_stokes_function_t x,
                                                           hh_stokes_function_t b, int level )
{
   return guarded( [&] {
      EPSS( solver ).prepare( EPS( op ) );
      EPSS( solver ).p->solve( EPS( op ), P1P1::fn( x ), P1P1::fn( b ), (uint_t) level );
   } );
}
HYTEG_HOST_API int hyteg_host_epsilon_stokes_minres_precondition( hh_epsilon_stokes_solver_t solver, hh_epsilon_stokes_t op, hh_stokes_function_t x,
                                                                  hh_stokes_function_t b, int level )
{
   return guarded( [&] {
      EPSS( solver ).prepare( EPS( op ) );
      EPSS( solver ).preconditioner->solve( EPS( op ), P1P1::fn( x ), P1P1::fn( b ), (uint_t) level );
   } );
}
HYTEG_HOST_API int hyteg_host_epsilon_stokes_minres_iterations( hh_epsilon_stokes_solver_t solver, int* iterations )
{
   return guarded( [&] { *iterations = (int) EPSS( solver ).p->getIterations(); } );
}
HYTEG_HOST_API int hyteg_host_epsilon_stokes_minres_destroy( hh_epsilon_stokes_solver_t solver )
{
   return guarded( [&] { delete static_cast< EpsilonStokesSolverH* >( solver ); } );
}

/* ---- P2 (single macro-cell) ---- */
HYTEG_HOST_API int hyteg_host_p2function_create( hh_storage_t s, const char* name, int minL, int maxL, hh_p2function_t* out )
{
   return guarded( [&] {
      *out = new P2FunctionH{ std::make_shared< P2Function< double > >( name, SP( s ), (uint_t) minL, (uint_t) maxL ) };
   } );
}
HYTEG_HOST_API int hyteg_host_p2function_destroy( hh_p2function_t f )
{
   return guarded( [&] { delete static_cast< P2FunctionH* >( f ); } );
}
HYTEG_HOST_API int hyteg_host_p2function_pointers( hh_p2function_t f, int local_cell, int level, double** vertex_dev, double** edge_dev )
{
   return guarded( [&] {
      *vertex_dev = F2( f ).getVertexDoFFunction().getCellPointer( (uint_t) local_cell, (uint_t) level );
      *edge_dev   = F2( f ).getEdgeCellPointer( (uint_t) local_cell, (uint_t) level );
   } );
}
HYTEG_HOST_API int hyteg_host_p2function_upload( hh_p2function_t f, int local_cell, int level, const double* vertex_host, const double* edge_host )
{
   return guarded( [&] {
      F2( f ).getVertexDoFFunction().copyCellFromHost( (uint_t) local_cell, (uint_t) level, vertex_host );
      F2( f ).copyEdgeFromHost( (uint_t) local_cell, (uint_t) level, edge_host );
   } );
}
HYTEG_HOST_API int hyteg_host_p2function_download( hh_p2function_t f, int local_cell, int level, double* vertex_host, double* edge_host )
{
   return guarded( [&] {
      F2( f ).getVertexDoFFunction().copyCellToHost( (uint_t) local_cell, (uint_t) level, vertex_host );
      F2( f ).copyEdgeToHost( (uint_t) local_cell, (uint_t) level, edge_host );
   } );
}
HYTEG_HOST_API int hyteg_host_p2function_interpolate_constant( hh_p2function_t f, double value, int level, int flag )
{
   return guarded( [&] { F2( f ).interpolate( value, (uint_t) level, DoFType( flag ) ); } );
}
HYTEG_HOST_API int hyteg_host_p2function_assign( hh_p2function_t dst, int n, const double* scalars, const hh_p2function_t* srcs, int level, int flag )
{
   return guarded( [&] { F2( dst ).assign( std::vector< double >( scalars, scalars + n ), refs2( n, srcs ), (uint_t) level, DoFType( flag ) ); } );
}
HYTEG_HOST_API int hyteg_host_p2function_add( hh_p2function_t dst, int n, const double* scalars, const hh_p2function_t* srcs, int level, int flag )
{
   return guarded( [&] { F2( dst ).add( std::vector< double >( scalars, scalars + n ), refs2( n, srcs ), (uint_t) level, DoFType( flag ) ); } );
}
HYTEG_HOST_API int hyteg_host_p2function_mult_elementwise( hh_p2function_t dst, int n, const hh_p2function_t* srcs, int level, int flag )
{
   return guarded( [&] { F2( dst ).multElementwise( refs2( n, srcs ), (uint_t) level, DoFType( flag ) ); } );
}
HYTEG_HOST_API int hyteg_host_p2function_dot( hh_p2function_t a, hh_p2function_t b, int level, int flag, double* result )
{
   return guarded( [&] { *result = F2( a ).dotGlobal( F2( b ), (uint_t) level, DoFType( flag ) ); } );
}
HYTEG_HOST_API int hyteg_host_p2_reduce( hh_p2function_t f, int level, int flag, int mpi_reduce, double* out )
{
   return guarded( [&] { reduceInto( F2( f ), level, flag, mpi_reduce, out ); } );
}
HYTEG_HOST_API int hyteg_host_p2operator_create( hh_storage_t s, int minL, int maxL, hh_p2operator_t* out )
{
   return guarded( [&] {
      *out = new P2OperatorH{ std::make_shared< P2ElementwiseLaplaceOperator >( SP( s ), (uint_t) minL, (uint_t) maxL ) };
   } );
}
HYTEG_HOST_API int hyteg_host_p2_prolongate( hh_p2function_t f, int sourceLevel, int flag, int add )
{
   return guarded( [&] {
      auto& fn = *static_cast< P2FunctionH* >( f )->p;
      if ( add )
         P2toP2QuadraticProlongation().prolongateAndAdd( fn, (uint_t) sourceLevel, DoFType( flag ) );
      else
         P2toP2QuadraticProlongation().prolongate( fn, (uint_t) sourceLevel, DoFType( flag ) );
   } );
}
HYTEG_HOST_API int hyteg_host_p2_restrict( hh_p2function_t f, int sourceLevel, int flag )
{
   return guarded( [&] { P2toP2QuadraticRestriction().restrict( *static_cast< P2FunctionH* >( f )->p, (uint_t) sourceLevel, DoFType( flag ) ); } );
}
HYTEG_HOST_API int hyteg_host_p2operator_create_constant( hh_storage_t s, int minL, int maxL, hh_p2operator_t* out )
{
   return guarded( [&] {
      *out = new P2OperatorH{ std::make_shared< P2ConstantLaplaceOperator >( SP( s ), (uint_t) minL, (uint_t) maxL ) };
   } );
}
HYTEG_HOST_API int hyteg_host_p2operator_constant_stencils( hh_p2operator_t op, int local_cell, int level, double* out, int capacity, int* count )
{
   return guarded( [&] {
      auto* c = dynamic_cast< P2ConstantLaplaceOperator* >( static_cast< P2OperatorH* >( op )->p.get() );
      if ( !c )
         throw std::runtime_error( "p2operator_constant_stencils: not a P2ConstantLaplaceOperator" );
      const auto& v = c->getInnerStencils( (uint_t) level, (uint_t) local_cell );
      *count        = (int) v.size();
      if ( capacity < (int) v.size() )
         throw std::runtime_error( "p2operator_constant_stencils: buffer too small" );
      std::copy( v.begin(), v.end(), out );
   } );
}
HYTEG_HOST_API int hyteg_host_p2operator_destroy( hh_p2operator_t op )
{
   return guarded( [&] { delete static_cast< P2OperatorH* >( op ); } );
}
HYTEG_HOST_API int hyteg_host_p2operator_element_matrices( hh_p2operator_t op, int local_cell, int level, double* out600 )
{
   return guarded( [&] {
      const auto& h = static_cast< P2OperatorH* >( op )->p->getElementMatrices( (uint_t) level, (uint_t) local_cell );
      std::copy( h.begin(), h.end(), out600 );
   } );
}
HYTEG_HOST_API int hyteg_host_p2operator_apply( hh_p2operator_t op, hh_p2function_t src, hh_p2function_t dst, int level, int flag, int update )
{
   return guarded( [&] { static_cast< P2OperatorH* >( op )->p->apply( F2( src ), F2( dst ), (uint_t) level, DoFType( flag ), UpdateType( update ) ); } );
}
/* P2 Jacobi smoother and geometric multigrid (P2ElementwiseOperator::smooth_jac, WeightedJacobiSmoother,
 * GeometricMultigridSolver with P2toP2Quadratic{Restriction,Prolongation}, CG on the coarsest level) */
HYTEG_HOST_API int hyteg_host_p2operator_compute_inverse_diagonal( hh_p2operator_t op )
{
   return guarded( [&] { static_cast< P2OperatorH* >( op )->p->computeInverseDiagonalOperatorValues(); } );
}
HYTEG_HOST_API int hyteg_host_p2operator_inverse_diagonal_copy( hh_p2operator_t op, hh_p2function_t dst, int level )
{
   return guarded( [&] { F2( dst ).assign( { 1.0 }, { *static_cast< P2OperatorH* >( op )->p->getInverseDiagonalValues() }, (uint_t) level, All ); } );
}
HYTEG_HOST_API int hyteg_host_p2operator_smooth_jac( hh_p2operator_t op, hh_p2function_t dst, hh_p2function_t rhs, hh_p2function_t src, double relax,
                                                     int level, int flag )
{
   return guarded( [&] { static_cast< P2OperatorH* >( op )->p->smooth_jac( F2( dst ), F2( rhs ), F2( src ), relax, (uint_t) level, DoFType( flag ) ); } );
}
HYTEG_HOST_API int hyteg_host_p2operator_smooth_sor( hh_p2operator_t op, hh_p2function_t dst, hh_p2function_t rhs, double relax, int level, int flag,
                                                     int backwards )
{
   return guarded( [&] {
      static_cast< P2OperatorH* >( op )->p->smooth_sor( F2( dst ), F2( rhs ), relax, (uint_t) level, DoFType( flag ), backwards != 0 );
   } );
}
HYTEG_HOST_API int hyteg_host_p2_gmg_create( hh_storage_t s, int minL, int maxL, int smootherKind, double relax, int pre, int post, int wcycle,
                                             int cgMaxIter, double cgTol, hh_p2solver_t* out )
{
   return guarded( [&] {
      using Op = P2ElementwiseLaplaceOperator;
      auto sm  = scalarSmoother< Op >( smootherKind, SP( s ), minL, maxL, relax );
      if ( !sm ) // every other code: SOR
         sm = std::make_shared< SORSmoother< Op > >( relax );
      *out = new P2SolverH{ makeGmg< Op, P2toP2QuadraticRestriction, P2toP2QuadraticProlongation >(
          SP( s ), sm, cgCoarse< Op >( SP( s ), minL, cgMaxIter, cgTol ), minL, maxL, pre, post, 0, cycleOf( wcycle ) ) };
   } );
}
HYTEG_HOST_API int hyteg_host_p2_fmg_create( hh_storage_t s, hh_p2solver_t gmg, int minL, int maxL, const unsigned* cyclesPerLevel, int nCycles,
                                             hh_level_callback_t postCycle, void* postCycleUser, hh_level_callback_t postProlongate,
                                             void* postProlongateUser, hh_p2solver_t* out )
{
   return guarded( [&] {
      using Op  = P2ElementwiseLaplaceOperator;
      using Gmg = GeometricMultigridSolver< Op, P2toP2QuadraticRestriction, P2toP2QuadraticProlongation >;
      auto g    = std::dynamic_pointer_cast< Gmg >( static_cast< P2SolverH* >( gmg )->p );
      if ( !g )
         throw std::runtime_error( "p2_fmg_create: not a geometric multigrid solver" );
      *out = new P2SolverH{ std::make_shared< FullMultigridSolver< Op, Gmg, P2toP2QuadraticProlongation > >(
          SP( s ), g, std::make_shared< P2toP2QuadraticProlongation >(), (uint_t) minL, (uint_t) maxL,
          fmgCycles( "p2_fmg_create", minL, maxL, cyclesPerLevel, nCycles ), levelCallback( postCycle, postCycleUser ),
          levelCallback( postProlongate, postProlongateUser ) ) };
   } );
}
HYTEG_HOST_API int hyteg_host_p2_chebyshev_estimate_radius( hh_p2operator_t op, int level, int maxIter, hh_p2function_t x, hh_p2function_t tmp,
                                                            double* radius )
{
   return guarded( [&] {
      const auto& A = *static_cast< P2OperatorH* >( op )->p;
      *radius       = chebyshev::estimateRadius( A, (uint_t) level, (uint_t) maxIter, F2( x ).getStorage(), F2( x ), F2( tmp ) );
   } );
}
HYTEG_HOST_API int hyteg_host_p2_chebyshev_create( hh_storage_t s, int minL, int maxL, int order, const double* radii, int nRadii, double upper,
                                                   double lower, hh_p2solver_t* out )
{
   return guarded(
       [&] { *out = new P2SolverH{ makeChebyshev< P2ElementwiseLaplaceOperator >( s, minL, maxL, order, radii, nRadii, upper, lower ) }; } );
}
HYTEG_HOST_API int hyteg_host_p2_gmg_create_chebyshev( hh_storage_t s, int minL, int maxL, int order, const double* radii, int nRadii, double upper,
                                                       double lower, int pre, int post, int wcycle, int cgMaxIter, double cgTol, hh_p2solver_t* out )
{
   return guarded( [&] {
      using Op = P2ElementwiseLaplaceOperator;
      auto sm  = makeChebyshev< Op >( s, minL, maxL, order, radii, nRadii, upper, lower );
      *out = new P2SolverH{ makeGmg< Op, P2toP2QuadraticRestriction, P2toP2QuadraticProlongation >(
          SP( s ), sm, cgCoarse< Op >( SP( s ), minL, cgMaxIter, cgTol ), minL, maxL, pre, post, 0, cycleOf( wcycle ) ) };
   } );
}
HYTEG_HOST_API int hyteg_host_p2_solver_solve( hh_p2solver_t solver, hh_p2operator_t op, hh_p2function_t x, hh_p2function_t b, int level )
{
   return guarded( [&] { static_cast< P2SolverH* >( solver )->p->solve( *static_cast< P2OperatorH* >( op )->p, F2( x ), F2( b ), (uint_t) level ); } );
}
HYTEG_HOST_API int hyteg_host_p2_solver_destroy( hh_p2solver_t solver )
{
   return guarded( [&] { delete static_cast< P2SolverH* >( solver ); } );
}
HYTEG_HOST_API int hyteg_host_p2_cg_create_preconditioned( hh_storage_t s, int minL, int maxL, int maxIter, double tol, hh_p2solver_t preconditioner,
                                                           hh_p2solver_t* out )
{
   return guarded( [&] {
      cgCreatePreconditioned< P2ElementwiseLaplaceOperator, P2SolverH >( "p2_cg_create_preconditioned", s, minL, maxL, maxIter, tol, preconditioner,
                                                                        out );
   } );
}
HYTEG_HOST_API int hyteg_host_p2_cg_iterations( hh_p2solver_t solver, int* iterations )
{
   return guarded( [&] { cgIterations< P2ElementwiseLaplaceOperator, P2SolverH >( "p2_cg_iterations", solver, iterations ); } );
}
HYTEG_HOST_API int hyteg_host_p2_smoother_create( hh_storage_t s, int minL, int maxL, int smoother, double relax, hh_p2solver_t* out )
{
   return guarded( [&] { smootherCreate< P2ElementwiseLaplaceOperator, P2SolverH >( "p2_smoother_create", s, minL, maxL, smoother, relax, out ); } );
}
HYTEG_HOST_API int hyteg_host_p2_cg_solve( hh_storage_t s, hh_p2operator_t op, hh_p2function_t x, hh_p2function_t b, int level, int maxIter,
                                           double tol, int* iterations )
{
   return guarded( [&] {
      CGSolver< P2ElementwiseLaplaceOperator > cg( SP( s ), (uint_t) level, (uint_t) level, (uint_t) maxIter, tol, tol );
      cg.solve( *static_cast< P2OperatorH* >( op )->p, F2( x ), F2( b ), (uint_t) level );
      if ( iterations )
         *iterations = (int) cg.getIterations();
   } );
}
}

/* ---- the generated variable-coefficient P2 operator: P2ElementwiseDivKGrad with a P2 coefficient, the solvers instantiated for it, and
 * P2ElementwiseMassOperator (p2divkgrad.hpp) ---- */
namespace {
using P2DivKGrad = operatorgeneration::P2ElementwiseDivKGrad;
using P2DkGmg    = GeometricMultigridSolver< P2DivKGrad, P2toP2QuadraticRestriction, P2toP2QuadraticProlongation >;
struct P2DivKGradH
{
   std::shared_ptr< P2Function< double > > k; // the operator holds a reference: the handle keeps the function alive
   std::shared_ptr< P2DivKGrad >           p;
};
struct P2DivKGradSolverH
{
   std::shared_ptr< Solver< P2DivKGrad > > p;
};
struct P2MassOperatorH
{
   std::shared_ptr< P2ElementwiseMassOperator > p;
};
P2DivKGrad& DK2( hh_p2divkgrad_t op )
{
   if ( !op )
      throw std::runtime_error( "null p2divkgrad operator" );
   return *static_cast< P2DivKGradH* >( op )->p;
}
std::shared_ptr< Solver< P2DivKGrad > > p2DivKGradSmoother( hh_storage_t s, int minL, int maxL, int code, double relax )
{
   if ( code == 0 )
      return std::make_shared< WeightedJacobiSmoother< P2DivKGrad > >( SP( s ), (uint_t) minL, (uint_t) maxL, relax );
   if ( code == -1 )
      return std::make_shared< IdentityPreconditioner< P2DivKGrad > >();
   throw std::runtime_error( "p2divkgrad_smoother_create: smoother 0 (weighted Jacobi) or -1 (identity)" );
}
} // namespace
HYTEG_HOST_API int hyteg_host_p2divkgrad_create( hh_storage_t s, int minL, int maxL, hh_p2function_t k, hh_p2divkgrad_t* out )
{
   return guarded( [&] {
      if ( !k || minL < 0 || maxL < minL )
         throw std::runtime_error( "p2divkgrad_create: needs a coefficient function and 0 <= min_level <= max_level" );
      auto h = std::make_unique< P2DivKGradH >();
      h->k   = static_cast< P2FunctionH* >( k )->p;
      h->p   = std::make_shared< P2DivKGrad >( SP( s ), (uint_t) minL, (uint_t) maxL, *h->k );
      *out   = h.release();
   } );
}
HYTEG_HOST_API int hyteg_host_p2divkgrad_destroy( hh_p2divkgrad_t op )
{
   return guarded( [&] { delete static_cast< P2DivKGradH* >( op ); } );
}
HYTEG_HOST_API int hyteg_host_p2divkgrad_apply( hh_p2divkgrad_t op, hh_p2function_t src, hh_p2function_t dst, int level, int flag, int update )
{
   return guarded( [&] { DK2( op ).apply( F2( src ), F2( dst ), (uint_t) level, DoFType( flag ), update ? Add : Replace ); } );
}
HYTEG_HOST_API int hyteg_host_p2divkgrad_gemv( hh_p2divkgrad_t op, double alpha, hh_p2function_t src, double beta, hh_p2function_t dst, int level,
                                               int flag )
{
   return guarded( [&] { DK2( op ).gemv( alpha, F2( src ), beta, F2( dst ), (uint_t) level, DoFType( flag ) ); } );
}
HYTEG_HOST_API int hyteg_host_p2divkgrad_compute_inverse_diagonal( hh_p2divkgrad_t op )
{
   return guarded( [&] { DK2( op ).computeInverseDiagonalOperatorValues(); } );
}
HYTEG_HOST_API int hyteg_host_p2divkgrad_inverse_diagonal_copy( hh_p2divkgrad_t op, hh_p2function_t dst, int level )
{
   return guarded( [&] { F2( dst ).assign( { 1.0 }, { *DK2( op ).getInverseDiagonalValues() }, (uint_t) level, All ); } );
}
HYTEG_HOST_API int hyteg_host_p2divkgrad_smooth_jac( hh_p2divkgrad_t op, hh_p2function_t dst, hh_p2function_t rhs, hh_p2function_t src, double relax,
                                                     int level, int flag )
{
   return guarded( [&] { DK2( op ).smooth_jac( F2( dst ), F2( rhs ), F2( src ), relax, (uint_t) level, DoFType( flag ) ); } );
}
HYTEG_HOST_API int hyteg_host_p2divkgrad_set_fused( hh_p2divkgrad_t op, int on )
{
   return guarded( [&] { DK2( op ).setFused( on != 0 ); } );
}
HYTEG_HOST_API int hyteg_host_p2divkgrad_chebyshev_fusable( hh_p2divkgrad_t op, int level, int* fusable )
{
   return guarded( [&] { *fusable = DK2( op ).chebyshevFusable( (uint_t) level ) ? 1 : 0; } );
}
HYTEG_HOST_API int hyteg_host_p2divkgrad_residual( hh_p2divkgrad_t op, hh_p2function_t x, hh_p2function_t b, hh_p2function_t r, int level, int flag )
{
   return guarded( [&] { DK2( op ).residual( F2( x ), F2( b ), F2( r ), (uint_t) level, DoFType( flag ) ); } );
}
HYTEG_HOST_API int hyteg_host_p2divkgrad_cg_create( hh_storage_t s, int minL, int maxL, int maxIter, double tol, hh_p2divkgrad_solver_t preconditioner,
                                                    hh_p2divkgrad_solver_t* out )
{
   return guarded( [&] {
      if ( preconditioner )
         cgCreatePreconditioned< P2DivKGrad, P2DivKGradSolverH >( "p2divkgrad_cg_create", s, minL, maxL, maxIter, tol, preconditioner, out );
      else
         *out = new P2DivKGradSolverH{ std::make_shared< CGSolver< P2DivKGrad > >( SP( s ), (uint_t) minL, (uint_t) maxL, (uint_t) maxIter, tol, tol ) };
   } );
}
HYTEG_HOST_API int hyteg_host_p2divkgrad_cg_iterations( hh_p2divkgrad_solver_t solver, int* iterations )
{
   return guarded( [&] { cgIterations< P2DivKGrad, P2DivKGradSolverH >( "p2divkgrad_cg_iterations", solver, iterations ); } );
}
HYTEG_HOST_API int hyteg_host_p2divkgrad_smoother_create( hh_storage_t s, int minL, int maxL, int smoother, double relax, hh_p2divkgrad_solver_t* out )
{
   return guarded( [&] { *out = new P2DivKGradSolverH{ p2DivKGradSmoother( s, minL, maxL, smoother, relax ) }; } );
}
HYTEG_HOST_API int hyteg_host_p2divkgrad_gmg_create( hh_storage_t s, int minL, int maxL, double relax, int pre, int post, int wcycle, int cgMaxIter,
                                                     double cgTol, hh_p2divkgrad_solver_t* out )
{
   return guarded( [&] {
      *out = new P2DivKGradSolverH{ makeGmg< P2DivKGrad, P2toP2QuadraticRestriction, P2toP2QuadraticProlongation >(
          SP( s ), p2DivKGradSmoother( s, minL, maxL, 0, relax ), cgCoarse< P2DivKGrad >( SP( s ), minL, cgMaxIter, cgTol ), minL, maxL, pre, post, 0,
          cycleOf( wcycle ) ) };
   } );
}
HYTEG_HOST_API int hyteg_host_p2divkgrad_chebyshev_estimate_radius( hh_p2divkgrad_t op, int level, int maxIter, hh_p2function_t x, hh_p2function_t tmp,
                                                                    double* radius )
{
   return guarded( [&] { *radius = chebyshev::estimateRadius( DK2( op ), (uint_t) level, (uint_t) maxIter, F2( x ).getStorage(), F2( x ), F2( tmp ) ); } );
}
HYTEG_HOST_API int hyteg_host_p2divkgrad_chebyshev_create( hh_storage_t s, int minL, int maxL, int order, const double* radii, int nRadii, double upper,
                                                           double lower, hh_p2divkgrad_solver_t* out )
{
   return guarded( [&] { *out = new P2DivKGradSolverH{ makeChebyshev< P2DivKGrad >( s, minL, maxL, order, radii, nRadii, upper, lower ) }; } );
}
HYTEG_HOST_API int hyteg_host_p2divkgrad_gmg_create_chebyshev( hh_storage_t s, int minL, int maxL, int order, const double* radii, int nRadii,
                                                               double upper, double lower, int pre, int post, int wcycle, int cgMaxIter, double cgTol,
                                                               hh_p2divkgrad_solver_t* out )
{
   return guarded( [&] {
      std::shared_ptr< Solver< P2DivKGrad > > sm = makeChebyshev< P2DivKGrad >( s, minL, maxL, order, radii, nRadii, upper, lower );
      *out = new P2DivKGradSolverH{ makeGmg< P2DivKGrad, P2toP2QuadraticRestriction, P2toP2QuadraticProlongation >(
          SP( s ), sm, cgCoarse< P2DivKGrad >( SP( s ), minL, cgMaxIter, cgTol ), minL, maxL, pre, post, 0, cycleOf( wcycle ) ) };
   } );
}
HYTEG_HOST_API int hyteg_host_p2divkgrad_fmg_create( hh_storage_t s, hh_p2divkgrad_solver_t gmg, int minL, int maxL, const unsigned* cyclesPerLevel,
                                                     int nCycles, hh_p2divkgrad_solver_t* out )
{
   return guarded( [&] {
      auto g = gmg ? std::dynamic_pointer_cast< P2DkGmg >( static_cast< P2DivKGradSolverH* >( gmg )->p ) : nullptr;
      if ( !g )
         throw std::runtime_error( "p2divkgrad_fmg_create: not a geometric multigrid solver" );
      *out = new P2DivKGradSolverH{ std::make_shared< FullMultigridSolver< P2DivKGrad, P2DkGmg, P2toP2QuadraticProlongation > >(
          SP( s ), g, std::make_shared< P2toP2QuadraticProlongation >(), (uint_t) minL, (uint_t) maxL,
          fmgCycles( "p2divkgrad_fmg_create", minL, maxL, cyclesPerLevel, nCycles ), levelCallback( nullptr, nullptr ), levelCallback( nullptr, nullptr ) ) };
   } );
}
HYTEG_HOST_API int hyteg_host_p2divkgrad_solver_solve( hh_p2divkgrad_solver_t solver, hh_p2divkgrad_t op, hh_p2function_t x, hh_p2function_t b, int level )
{
   return guarded( [&] { static_cast< P2DivKGradSolverH* >( solver )->p->solve( DK2( op ), F2( x ), F2( b ), (uint_t) level ); } );
}
HYTEG_HOST_API int hyteg_host_p2divkgrad_solver_destroy( hh_p2divkgrad_solver_t solver )
{
   return guarded( [&] { delete static_cast< P2DivKGradSolverH* >( solver ); } );
}
HYTEG_HOST_API int hyteg_host_p2massoperator_create( hh_storage_t s, int minL, int maxL, hh_p2massoperator_t* out )
{
   return guarded( [&] { *out = new P2MassOperatorH{ std::make_shared< P2ElementwiseMassOperator >( SP( s ), (uint_t) minL, (uint_t) maxL ) }; } );
}
HYTEG_HOST_API int hyteg_host_p2massoperator_apply( hh_p2massoperator_t op, hh_p2function_t src, hh_p2function_t dst, int level, int flag, int update )
{
   return guarded( [&] {
      if ( !op )
         throw std::runtime_error( "null p2 mass operator" );
      static_cast< P2MassOperatorH* >( op )->p->apply( F2( src ), F2( dst ), (uint_t) level, DoFType( flag ), UpdateType( update ) );
   } );
}
HYTEG_HOST_API int hyteg_host_p2massoperator_destroy( hh_p2massoperator_t op )
{
   return guarded( [&] { delete static_cast< P2MassOperatorH* >( op ); } );
}


/* ---- P2-P1 Taylor-Hood Stokes (taylorhood.hpp) ---- */
HYTEG_HOST_API int hyteg_host_th_function_create( hh_storage_t s, const char* name, int minL, int maxL, hh_th_function_t* out )
{
   return TH::functionCreate( s, name, minL, maxL, out );
}
HYTEG_HOST_API int hyteg_host_th_function_destroy( hh_th_function_t f ) { return TH::destroy< TH::FunctionHandle >( f ); }
HYTEG_HOST_API int hyteg_host_th_function_velocity( hh_th_function_t f, int k, hh_p2function_t* out )
{
   return guarded( [&] {
      if ( k < 0 || k > 2 )
         throw std::runtime_error( "th_function_velocity: k = 0, 1, 2" );
      *out = TH::velocityView( f, k );
   } );
}
HYTEG_HOST_API int hyteg_host_th_function_pressure( hh_th_function_t f, hh_function_t* out )
{
   return guarded( [&] { *out = TH::pressureView( f ); } );
}
HYTEG_HOST_API int hyteg_host_th_function_assign( hh_th_function_t dst, int n, const double* scalars, const hh_th_function_t* fs, int level, int flag )
{
   return TH::functionAssign( dst, n, scalars, fs, level, flag );
}
HYTEG_HOST_API int hyteg_host_th_function_interpolate_constant( hh_th_function_t f, double value, int level, int flag )
{
   return guarded( [&] { TH::fn( f ).interpolate( value, (uint_t) level, DoFType( flag ) ); } );
}
HYTEG_HOST_API int hyteg_host_th_function_dot( hh_th_function_t a, hh_th_function_t b, int level, int flag, double* out )
{
   return TH::functionDot( a, b, level, flag, out );
}
HYTEG_HOST_API int hyteg_host_th_operator_create( hh_storage_t s, int minL, int maxL, hh_th_operator_t* out )
{
   return TH::operatorCreate( s, minL, maxL, out );
}
HYTEG_HOST_API int hyteg_host_th_operator_destroy( hh_th_operator_t op ) { return TH::destroy< TH::OperatorHandle >( op ); }
HYTEG_HOST_API int hyteg_host_th_operator_apply( hh_th_operator_t op, hh_th_function_t src, hh_th_function_t dst, int level, int flag )
{
   return TH::operatorApply( op, src, dst, level, flag );
}
// single blocks, for the parity tests: which = 0 div (velocity of src -> pressure of dst), 1 divT (pressure of src -> velocity of dst)
HYTEG_HOST_API int hyteg_host_th_operator_apply_block( hh_th_operator_t op, int which, hh_th_function_t src, hh_th_function_t dst, int level, int flag )
{
   return guarded( [&] {
      auto& A = TH::op( op );
      if ( which == 0 )
         A.div.apply( TH::fn( src ).uvw(), TH::fn( dst ).p(), (uint_t) level, DoFType( flag ), Replace );
      else if ( which == 1 )
         A.divT.apply( TH::fn( src ).p(), TH::fn( dst ).uvw(), (uint_t) level, DoFType( flag ), Replace );
      else
         throw std::runtime_error( "th_operator_apply_block: which = 0 (div) or 1 (divT)" );
   } );
}
// GeometricMultigridSolver< P2P1TaylorHoodStokesOperator > as tests/hyteg/convergence/P2P1Stokes3DUzawaConvergenceTest.cpp:150-163 composes it:
// UzawaSmoother( relax ) over StokesVelocityBlockBlockDiagonalPreconditioner( GaussSeidelSmoother ), P2P1StokesToP2P1Stokes transfer with
// projectMean after the restriction, V( pre, post ) + increment; coarse grid: MinResSolver preconditioned with
// StokesPressureBlockPreconditioner< ., P1LumpedInvMassOperator > (the reference's test uses PETSc's LU there)
HYTEG_HOST_API int hyteg_host_th_gmg_create( hh_storage_t s, int minL, int maxL, double uzawa_relax, int pre, int post, int increment,
                                             int coarse_max_iter, double coarse_rel_tol, hh_th_solver_t* out )
{
   return guarded( [&] {
      using Op     = P2P1TaylorHoodStokesOperator;
      auto storage = SP( s );
      auto gs      = std::make_shared< GaussSeidelSmoother< P2ConstantLaplaceOperator > >();
      auto vel     = std::make_shared< StokesVelocityBlockBlockDiagonalPreconditioner< Op > >( storage, gs );
      auto uzawa   = std::make_shared< UzawaSmoother< Op > >( storage, vel, (uint_t) minL, (uint_t) maxL, uzawa_relax );
      auto coarse  = TH::pressureMinres( storage, minL, minL, coarse_max_iter, coarse_rel_tol );
      *out         = new TH::SolverHandle{ makeGmg< Op, P2P1StokesToP2P1StokesRestriction, P2P1StokesToP2P1StokesProlongation >(
          storage, uzawa, coarse, minL, maxL, pre, post, increment, CycleType::VCYCLE, true ) };
   } );
}
HYTEG_HOST_API int hyteg_host_th_minres_create( hh_storage_t s, int minL, int maxL, int max_iter, double rel_tol, hh_th_solver_t* out )
{
   return guarded( [&] {
      *out = new TH::SolverHandle{ TH::pressureMinres( SP( s ), minL, maxL, max_iter, rel_tol ) };
   } );
}
HYTEG_HOST_API int hyteg_host_th_solver_solve( hh_th_solver_t solver, hh_th_operator_t op, hh_th_function_t x, hh_th_function_t b, int level )
{
   return TH::solverSolve( solver, op, x, b, level );
}
HYTEG_HOST_API int hyteg_host_th_solver_destroy( hh_th_solver_t solver ) { return TH::destroy< TH::SolverHandle >( solver ); }
HYTEG_HOST_API int hyteg_host_th_project_pressure_mean( hh_th_function_t f, int level )
{
   return guarded( [&] { projectMean( TH::fn( f ).p(), (uint_t) level ); } );
}
// the 10 x 10 element matrix (FEniCS ordering) a mixed block hands to the P2 kernel: which = 0 div (edge rows zero), 1 divT (edge
// columns zero), component k, tetrahedron coords[4][3] -- for the pins against the reference's FEniCS forms
HYTEG_HOST_API int hyteg_host_th_form_element_matrix( int which, int k, const double* coords12, double* out100 )
{
   return guarded( [&] {
      std::array< Point3D, 4 > c;
      for ( int v = 0; v < 4; ++v )
         for ( int r = 0; r < 3; ++r )
            c[v][r] = coords12[3 * v + r];
      if ( k < 0 || k > 2 || which < 0 || which > 1 )
         throw std::runtime_error( "th_form_element_matrix: which = 0, 1; k = 0, 1, 2" );
      if ( which == 0 )
         k == 0 ? forms::P2ToP1DivForm< 0 >::integrateAll( c, out100 ) : ( k == 1 ? forms::P2ToP1DivForm< 1 >::integrateAll( c, out100 ) : forms::P2ToP1DivForm< 2 >::integrateAll( c, out100 ) );
      else
         k == 0 ? forms::P1ToP2DivTForm< 0 >::integrateAll( c, out100 ) : ( k == 1 ? forms::P1ToP2DivTForm< 1 >::integrateAll( c, out100 ) : forms::P1ToP2DivTForm< 2 >::integrateAll( c, out100 ) );
   } );
}

/* ---- variable-viscosity Taylor-Hood Stokes: P2ViscousBlockEpsilonOperator, P2P1StokesEpsilonOperator and the solvers instantiated for
 * them (p2epsilon.hpp) ---- */
namespace {
using P2Epsilon       = operatorgeneration::P2ViscousBlockEpsilonOperator;
using P2EpsilonStokes = operatorgeneration::P2P1StokesEpsilonOperator;
struct P2EpsilonH
{
   std::shared_ptr< P2Function< double > > mu; // the operator holds a reference: the handle keeps the function alive
   std::shared_ptr< P2Epsilon >            p;
   P2FunctionH                             invDiag[3]; // borrowed views
};
struct P2EpsilonSolverH
{
   std::shared_ptr< Solver< P2Epsilon > > p;
};
struct P2EpsilonStokesH
{
   std::shared_ptr< P2Function< double > > mu;
   std::shared_ptr< P2EpsilonStokes >      p;
};
struct P2EpsilonStokesSolverH
{
   std::shared_ptr< P2Function< double > >            mu; // of the viscosity-weighted preconditioner, or null
   std::shared_ptr< Solver< P2EpsilonStokes > >       preconditioner;
   std::shared_ptr< MinResSolver< P2EpsilonStokes > > p;
   bool                                               smoothsVelocity = false; // its preconditioner reads the velocity operator's inverse diagonals
   // assembled on first use: the Stokes operator does not assemble them itself (the pressure preconditioners never read them)
   void prepare( P2EpsilonStokes& op ) const
   {
      if ( smoothsVelocity && !op.viscOp.hasInverseDiagonalValues() )
         op.viscOp.computeInverseDiagonalOperatorValues();
   }
};
P2Epsilon& EP2( hh_p2epsilon_t op )
{
   if ( !op )
      throw std::runtime_error( "null p2 epsilon operator" );
   return *static_cast< P2EpsilonH* >( op )->p;
}
P2EpsilonStokes& EPS2( hh_th_epsilon_t op )
{
   if ( !op )
      throw std::runtime_error( "null Taylor-Hood epsilon Stokes operator" );
   return *static_cast< P2EpsilonStokesH* >( op )->p;
}
P2EpsilonStokesSolverH& EPSS2( hh_th_epsilon_solver_t solver )
{
   if ( !solver )
      throw std::runtime_error( "null Taylor-Hood epsilon Stokes solver" );
   return *static_cast< P2EpsilonStokesSolverH* >( solver );
}
// three function handles as one P2VectorFunction (a view: the handles keep the components)
P2VectorFunction< double > vectorOf2( const hh_p2function_t* f )
{
   if ( !f || !f[0] || !f[1] || !f[2] )
      throw std::runtime_error( "p2 epsilon: three component functions" );
   return P2VectorFunction< double >(
       { static_cast< P2FunctionH* >( f[0] )->p, static_cast< P2FunctionH* >( f[1] )->p, static_cast< P2FunctionH* >( f[2] )->p } );
}
std::shared_ptr< P2Function< double > > viscosityOf2( const char* who, hh_p2function_t mu, int minL, int maxL )
{
   if ( !mu || minL < 0 || maxL < minL )
      throw std::runtime_error( std::string( who ) + ": needs a viscosity function and 0 <= min_level <= max_level" );
   return static_cast< P2FunctionH* >( mu )->p;
}
// a multigrid cycle on P2 vector functions: the quadratic P2 transfer on every component, CG on the coarsest level
std::shared_ptr< Solver< P2Epsilon > > p2EpsilonGmg( hh_storage_t s, std::shared_ptr< Solver< P2Epsilon > > smoother, int minL, int maxL, int pre, int post,
                                                     int wcycle, int cgMaxIter, double cgTol )
{
   return makeGmg< P2Epsilon, P2toP2QuadraticVectorRestriction, P2toP2QuadraticVectorProlongation >(
       SP( s ), smoother, cgCoarse< P2Epsilon >( SP( s ), minL, cgMaxIter, cgTol ), minL, maxL, pre, post, 0, cycleOf( wcycle ) );
}
// chebyshev::estimateRadius from a start vector of incommensurate waves (components along every eigenvector)
double p2EpsilonRadius( const P2Epsilon& op, uint_t level, uint_t iterations )
{
   auto                       storage = op.getStorage();
   P2VectorFunction< double > x( "p2epsilon_radius_x", storage, level, level ), tmp( "p2epsilon_radius_tmp", storage, level, level );
   x.interpolate( { []( const Point3D& q ) { return std::sin( 7.3 * q[0] + 3.1 * q[1] + 1.7 * q[2] + 0.4 ); },
                    []( const Point3D& q ) { return std::cos( 2.9 * q[0] - 6.1 * q[1] + 4.3 * q[2] ); },
                    []( const Point3D& q ) { return std::sin( 5.3 * q[0] * q[1] - 3.7 * q[2] + 1.1 ); } },
                  level, All );
   return chebyshev::estimateRadius( op, level, iterations, storage, x, tmp );
}
} // namespace
HYTEG_HOST_API int hyteg_host_p2epsilon_create( hh_storage_t s, int minL, int maxL, hh_p2function_t mu, hh_p2epsilon_t* out )
{
   return guarded( [&] {
      auto h = std::make_unique< P2EpsilonH >();
      h->mu  = viscosityOf2( "p2epsilon_create", mu, minL, maxL );
      h->p   = std::make_shared< P2Epsilon >( SP( s ), (uint_t) minL, (uint_t) maxL, *h->mu );
      *out   = h.release();
   } );
}
HYTEG_HOST_API int hyteg_host_p2epsilon_destroy( hh_p2epsilon_t op )
{
   return guarded( [&] { delete static_cast< P2EpsilonH* >( op ); } );
}
HYTEG_HOST_API int hyteg_host_p2epsilon_apply( hh_p2epsilon_t op, const hh_p2function_t* src, const hh_p2function_t* dst, int level, int flag, int update )
{
   return guarded( [&] { EP2( op ).apply( vectorOf2( src ), vectorOf2( dst ), (uint_t) level, DoFType( flag ), update ? Add : Replace ); } );
}
HYTEG_HOST_API int hyteg_host_p2epsilon_gemv( hh_p2epsilon_t op, double alpha, const hh_p2function_t* src, double beta, const hh_p2function_t* dst,
                                              int level, int flag )
{
   return guarded( [&] { EP2( op ).gemv( alpha, vectorOf2( src ), beta, vectorOf2( dst ), (uint_t) level, DoFType( flag ) ); } );
}
HYTEG_HOST_API int hyteg_host_p2epsilon_compute_inverse_diagonal( hh_p2epsilon_t op )
{
   return guarded( [&] { EP2( op ).computeInverseDiagonalOperatorValues(); } );
}
HYTEG_HOST_API int hyteg_host_p2epsilon_inverse_diagonal( hh_p2epsilon_t op, hh_p2function_t* out )
{
   return guarded( [&] {
      auto*      h = static_cast< P2EpsilonH* >( op );
      const auto d = EP2( op ).getInverseDiagonalValues();
      for ( int k = 0; k < 3; ++k )
      {
         h->invDiag[k].p = viewOf( d, ( *d )[(uint_t) k] );
         out[k]          = &h->invDiag[k];
      }
   } );
}
HYTEG_HOST_API int hyteg_host_p2epsilon_smooth_jac( hh_p2epsilon_t op, const hh_p2function_t* dst, const hh_p2function_t* rhs, const hh_p2function_t* src,
                                                    double relax, int level, int flag )
{
   return guarded( [&] { EP2( op ).smooth_jac( vectorOf2( dst ), vectorOf2( rhs ), vectorOf2( src ), relax, (uint_t) level, DoFType( flag ) ); } );
}
HYTEG_HOST_API int hyteg_host_p2epsilon_set_fused( hh_p2epsilon_t op, int on )
{
   return guarded( [&] { EP2( op ).setFused( on != 0 ); } );
}
HYTEG_HOST_API int hyteg_host_p2epsilon_chebyshev_fusable( hh_p2epsilon_t op, int level, int* fusable )
{
   return guarded( [&] { *fusable = EP2( op ).chebyshevFusable( (uint_t) level ) ? 1 : 0; } );
}
HYTEG_HOST_API int hyteg_host_p2epsilon_residual( hh_p2epsilon_t op, const hh_p2function_t* x, const hh_p2function_t* b, const hh_p2function_t* r, int level,
                                                  int flag )
{
   return guarded( [&] { EP2( op ).residual( vectorOf2( x ), vectorOf2( b ), vectorOf2( r ), (uint_t) level, DoFType( flag ) ); } );
}
HYTEG_HOST_API int hyteg_host_p2epsilon_cg_create( hh_storage_t s, int minL, int maxL, int maxIter, double tol, hh_p2epsilon_solver_t preconditioner,
                                                   hh_p2epsilon_solver_t* out )
{
   return guarded( [&] {
      if ( preconditioner )
         cgCreatePreconditioned< P2Epsilon, P2EpsilonSolverH >( "p2epsilon_cg_create", s, minL, maxL, maxIter, tol, preconditioner, out );
      else
         *out = new P2EpsilonSolverH{ std::make_shared< CGSolver< P2Epsilon > >( SP( s ), (uint_t) minL, (uint_t) maxL, (uint_t) maxIter, tol, tol ) };
   } );
}
HYTEG_HOST_API int hyteg_host_p2epsilon_cg_iterations( hh_p2epsilon_solver_t solver, int* iterations )
{
   return guarded( [&] { cgIterations< P2Epsilon, P2EpsilonSolverH >( "p2epsilon_cg_iterations", solver, iterations ); } );
}
HYTEG_HOST_API int hyteg_host_p2epsilon_smoother_create( hh_storage_t s, int minL, int maxL, int smoother, double relax, hh_p2epsilon_solver_t* out )
{
   return guarded( [&] {
      if ( smoother == 0 )
         *out = new P2EpsilonSolverH{ std::make_shared< WeightedJacobiSmoother< P2Epsilon > >( SP( s ), (uint_t) minL, (uint_t) maxL, relax ) };
      else if ( smoother == -1 )
         *out = new P2EpsilonSolverH{ std::make_shared< IdentityPreconditioner< P2Epsilon > >() };
      else
         throw std::runtime_error( "p2epsilon_smoother_create: smoother 0 (weighted Jacobi) or -1 (identity); the operator has no SOR sweep" );
   } );
}
HYTEG_HOST_API int hyteg_host_p2epsilon_chebyshev_estimate_radius( hh_p2epsilon_t op, int level, int maxIter, double* radius )
{
   return guarded( [&] { *radius = p2EpsilonRadius( EP2( op ), (uint_t) level, (uint_t) maxIter ); } );
}
HYTEG_HOST_API int hyteg_host_p2epsilon_chebyshev_create( hh_storage_t s, int minL, int maxL, int order, const double* radii, int nRadii, double upper,
                                                          double lower, hh_p2epsilon_solver_t* out )
{
   return guarded( [&] { *out = new P2EpsilonSolverH{ makeChebyshev< P2Epsilon >( s, minL, maxL, order, radii, nRadii, upper, lower ) }; } );
}
HYTEG_HOST_API int hyteg_host_p2epsilon_gmg_create( hh_storage_t s, int minL, int maxL, double relax, int pre, int post, int wcycle, int cgMaxIter,
                                                    double cgTol, hh_p2epsilon_solver_t* out )
{
   return guarded( [&] {
      std::shared_ptr< Solver< P2Epsilon > > sm = std::make_shared< WeightedJacobiSmoother< P2Epsilon > >( SP( s ), (uint_t) minL, (uint_t) maxL, relax );
      *out = new P2EpsilonSolverH{ p2EpsilonGmg( s, sm, minL, maxL, pre, post, wcycle, cgMaxIter, cgTol ) };
   } );
}
HYTEG_HOST_API int hyteg_host_p2epsilon_gmg_create_chebyshev( hh_storage_t s, int minL, int maxL, int order, const double* radii, int nRadii, double upper,
                                                              double lower, int pre, int post, int wcycle, int cgMaxIter, double cgTol,
                                                              hh_p2epsilon_solver_t* out )
{
   return guarded( [&] {
      *out = new P2EpsilonSolverH{
          p2EpsilonGmg( s, makeChebyshev< P2Epsilon >( s, minL, maxL, order, radii, nRadii, upper, lower ), minL, maxL, pre, post, wcycle, cgMaxIter, cgTol ) };
   } );
}
HYTEG_HOST_API int hyteg_host_p2epsilon_solver_solve( hh_p2epsilon_solver_t solver, hh_p2epsilon_t op, const hh_p2function_t* x, const hh_p2function_t* b,
                                                      int level )
{
   return guarded( [&] {
      if ( !solver )
         throw std::runtime_error( "null p2 epsilon solver" );
      static_cast< P2EpsilonSolverH* >( solver )->p->solve( EP2( op ), vectorOf2( x ), vectorOf2( b ), (uint_t) level );
   } );
}
HYTEG_HOST_API int hyteg_host_p2epsilon_solver_destroy( hh_p2epsilon_solver_t solver )
{
   return guarded( [&] { delete static_cast< P2EpsilonSolverH* >( solver ); } );
}

HYTEG_HOST_API int hyteg_host_th_epsilon_create( hh_storage_t s, int minL, int maxL, hh_p2function_t mu, hh_th_epsilon_t* out )
{
   return guarded( [&] {
      auto h = std::make_unique< P2EpsilonStokesH >();
      h->mu  = viscosityOf2( "th_epsilon_create", mu, minL, maxL );
      h->p   = std::make_shared< P2EpsilonStokes >( SP( s ), (uint_t) minL, (uint_t) maxL, *h->mu );
      *out   = h.release();
   } );
}
HYTEG_HOST_API int hyteg_host_th_epsilon_destroy( hh_th_epsilon_t op )
{
   return guarded( [&] { delete static_cast< P2EpsilonStokesH* >( op ); } );
}
HYTEG_HOST_API int hyteg_host_th_epsilon_apply( hh_th_epsilon_t op, hh_th_function_t src, hh_th_function_t dst, int level, int flag )
{
   return guarded( [&] { EPS2( op ).apply( TH::fn( src ), TH::fn( dst ), (uint_t) level, DoFType( flag ) ); } );
}
// MinResSolver< P2P1StokesEpsilonOperator >; preconditioner 0 identity, 1 StokesPressureBlockPreconditioner< ., P1LumpedInvMassOperator >
// (solvertemplates::stokesMinResSolver, StokesSolverTemplates.hpp:54-69), 2 the same weighted with mu at the vertex DoFs
HYTEG_HOST_API int hyteg_host_th_epsilon_minres_create( hh_storage_t s, int minL, int maxL, int max_iter, double rel_tol, int preconditioner,
                                                        hh_p2function_t mu, hh_th_epsilon_solver_t* out )
{
   return guarded( [&] {
      auto storage = SP( s );
      auto h       = std::make_unique< P2EpsilonStokesSolverH >();
      if ( preconditioner == 0 )
         h->preconditioner = std::make_shared< IdentityPreconditioner< P2EpsilonStokes > >();
      else if ( preconditioner == 1 )
         h->preconditioner =
             std::make_shared< StokesPressureBlockPreconditioner< P2EpsilonStokes, P1LumpedInvMassOperator > >( storage, (uint_t) minL, (uint_t) maxL );
      else if ( preconditioner == 2 )
      {
         h->mu             = viscosityOf2( "th_epsilon_minres_create (viscosity-weighted preconditioner)", mu, minL, maxL );
         h->preconditioner = std::make_shared< StokesViscosityWeightedPressureBlockPreconditioner< P2EpsilonStokes > >(
             storage, (uint_t) minL, (uint_t) maxL, h->mu->getVertexDoFFunction() );
      }
      else
         throw std::runtime_error( "th_epsilon_minres_create: unknown preconditioner" );
      h->p = std::make_shared< MinResSolver< P2EpsilonStokes > >( storage, (uint_t) minL, (uint_t) maxL, (uint_t) max_iter, rel_tol, 1e-16,
                                                                  h->preconditioner );
      *out = h.release();
   } );
}
// MinResSolver preconditioned with StokesVectorBlockDiagonalPreconditioner: velocityCycles multigrid V-cycles on the P2 epsilon operator
// (smoother 0 weighted Jacobi( relax ), 1 Chebyshev( order; radii: none = estimated per level here, one, or one per level ); pre = post
// steps, CG on the coarsest level, levels velocityMinL .. maxL) and the lumped inverse mass on the pressure, weighted with mu at the vertex
// DoFs if viscosityWeighted.  mu: the viscosity of the operator the solver will be used with (the radii are estimated on an operator
// built from it).
HYTEG_HOST_API int hyteg_host_th_epsilon_minres_create_block( hh_storage_t s, int minL, int maxL, int max_iter, double rel_tol, int viscosityWeighted,
                                                              hh_p2function_t mu, int velocityMinL, int velocityCycles, int smoother, int order,
                                                              const double* radii, int nRadii, double relax, int pre, int post, int cgMaxIter,
                                                              double cgTol, hh_th_epsilon_solver_t* out )
{
   return guarded( [&] {
      const char* who     = "th_epsilon_minres_create_block";
      auto        storage = SP( s );
      auto        h       = std::make_unique< P2EpsilonStokesSolverH >();
      // MINRES needs a symmetric positive definite preconditioner
      if ( smoother != 0 && smoother != 1 )
         throw std::runtime_error( std::string( who ) + ": smoother 0 (weighted Jacobi) or 1 (Chebyshev); an SOR sweep is not symmetric" );
      if ( pre != post || pre < 1 )
         throw std::runtime_error( std::string( who ) + ": a symmetric cycle needs pre = post >= 1 smoothing steps" );
      if ( velocityCycles < 1 )
         throw std::runtime_error( std::string( who ) + ": velocity_cycles >= 1" );
      if ( velocityMinL < minL || velocityMinL > maxL )
         throw std::runtime_error( std::string( who ) + ": min_level <= velocity_min_level <= max_level" );
      h->mu = viscosityOf2( who, mu, minL, maxL );
      std::shared_ptr< Solver< P2Epsilon > > sm;
      if ( smoother == 0 )
         sm = std::make_shared< WeightedJacobiSmoother< P2Epsilon > >( storage, (uint_t) velocityMinL, (uint_t) maxL, relax );
      else
      {
         std::vector< double > rho( radii, radii + ( radii ? nRadii : 0 ) );
         if ( rho.empty() )
         {
            P2Epsilon probe( storage, (uint_t) velocityMinL, (uint_t) maxL, *h->mu );
            probe.computeInverseDiagonalOperatorValues();
            for ( int l = velocityMinL; l <= maxL; ++l )
               rho.push_back( p2EpsilonRadius( probe, (uint_t) l, 20 ) );
         }
         sm = makeChebyshev< P2Epsilon >( s, velocityMinL, maxL, order, rho.data(), (int) rho.size(), 1.2, 0.3 );
      }
      auto velocity      = p2EpsilonGmg( s, sm, velocityMinL, maxL, pre, post, 0, cgMaxIter, cgTol );
      h->smoothsVelocity = true;
      if ( viscosityWeighted )
         h->preconditioner =
             std::make_shared< StokesVectorBlockDiagonalPreconditioner< P2EpsilonStokes, Solver< P2Epsilon >, P1ViscosityWeightedLumpedInvMassOperator > >(
                 velocity,
                 std::make_shared< P1ViscosityWeightedLumpedInvMassOperator >( storage, (uint_t) minL, (uint_t) maxL, h->mu->getVertexDoFFunction() ),
                 (uint_t) velocityCycles );
      else
         h->preconditioner = std::make_shared< StokesVectorBlockDiagonalPreconditioner< P2EpsilonStokes, Solver< P2Epsilon >, P1LumpedInvMassOperator > >(
             velocity, std::make_shared< P1LumpedInvMassOperator >( storage, (uint_t) minL, (uint_t) maxL ), (uint_t) velocityCycles );
      h->p = std::make_shared< MinResSolver< P2EpsilonStokes > >( storage, (uint_t) minL, (uint_t) maxL, (uint_t) max_iter, rel_tol, 1e-16,
                                                                  h->preconditioner );
      *out = h.release();
   } );
}
HYTEG_HOST_API int hyteg_host_th_epsilon_minres_solve( hh_th_epsilon_solver_t solver, hh_th_epsilon_t op, hh_th_function_t x, hh_th_function_t b, int level )
{
   return guarded( [&] {
      EPSS2( solver ).prepare( EPS2( op ) );
      EPSS2( solver ).p->solve( EPS2( op ), TH::fn( x ), TH::fn( b ), (uint_t) level );
   } );
}
HYTEG_HOST_API int hyteg_host_th_epsilon_minres_precondition( hh_th_epsilon_solver_t solver, hh_th_epsilon_t op, hh_th_function_t x, hh_th_function_t b,
                                                              int level )
{
   return guarded( [&] {
      EPSS2( solver ).prepare( EPS2( op ) );
      EPSS2( solver ).preconditioner->solve( EPS2( op ), TH::fn( x ), TH::fn( b ), (uint_t) level );
   } );
}
HYTEG_HOST_API int hyteg_host_th_epsilon_minres_iterations( hh_th_epsilon_solver_t solver, int* iterations )
{
   return guarded( [&] { *iterations = (int) EPSS2( solver ).p->getIterations(); } );
}
HYTEG_HOST_API int hyteg_host_th_epsilon_minres_destroy( hh_th_epsilon_solver_t solver )
{
   return guarded( [&] { delete static_cast< P2EpsilonStokesSolverH* >( solver ); } );
}
