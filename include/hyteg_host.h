/*
 * hyteg_host.h -- C facade over the C++ host layer (hyteg_amd/host/hyteg_host.hpp) for non-C++ callers
 * (the pytest suite, bench.py and the torch.distributed driver use it through ctypes).  The C++ classes
 * carry the reference's names (PrimitiveStorage, P1Function, P1ConstantLaplaceOperator, P1toP1Linear*,
 * GeometricMultigridSolver ...); this header only flattens them to handles.  Library: libhyteg_host.so,
 * which itself calls nothing but libhyteg_hip.so (include/hyteg_hip.h).
 *
 * All functions return 0 on success, non-zero on failure (hyteg_host_last_error() has the message); the
 * reference would WALBERLA_ABORT.  Handles are opaque pointers.  DoFType flags and UpdateType are the integer
 * values of src/hyteg/types/types.hpp:29-44 (Inner = 1, DirichletBoundary = 2, NeumannBoundary = 4, All = 15).
 */
#ifndef HYTEG_HOST_H
#define HYTEG_HOST_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
#if defined( HYTEG_HOST_BUILDING )
#define HYTEG_HOST_API __attribute__( ( visibility( "default" ) ) )
#else
#define HYTEG_HOST_API
#endif

typedef void* hh_storage_t;
typedef void* hh_function_t;
typedef void* hh_operator_t;
typedef void* hh_solver_t;
typedef void* hh_p2function_t;
typedef void* hh_p2operator_t;
typedef void* hh_elementwise_t;
typedef void* hh_stokes_function_t;
typedef void* hh_stokes_operator_t;
typedef void* hh_stokes_solver_t;
typedef void* hh_boundary_condition_t;

HYTEG_HOST_API const char* hyteg_host_last_error( void );

/* ---- PrimitiveStorage ---- */
HYTEG_HOST_API int hyteg_host_storage_from_gmsh( const char* path, int rank, int nranks, hh_storage_t* out );
HYTEG_HOST_API int hyteg_host_storage_from_arrays( int nvertices, const double* xyz, int ncells, const int* cells, int rank, int nranks, hh_storage_t* out );
HYTEG_HOST_API int hyteg_host_storage_destroy( hh_storage_t s );
/* counts[0..5] = global cells, faces, edges, vertices, local cells, ranks */
HYTEG_HOST_API int hyteg_host_storage_counts( hh_storage_t s, int* counts );
HYTEG_HOST_API int hyteg_host_storage_local_cell( hh_storage_t s, int local_index, int* global_id, double* coords12, double* nnc14 );
HYTEG_HOST_API int hyteg_host_storage_mask( hh_storage_t s, int local_index, int flag, int owned, unsigned* mask );
/* PrimitiveStorage::setBoundaryType: re-types mesh flag 1 of the storage's default boundary condition (create0123BC) */
HYTEG_HOST_API int hyteg_host_storage_set_boundary_type( hh_storage_t s, int dof_type );
/* the mask under a boundary condition of its own (bc == NULL: the storage's default one):
 * bc.getBoundaryType( primitive.getMeshBoundaryFlag() ) tested against `flag`, P1Operator.hpp:301-303 */
HYTEG_HOST_API int hyteg_host_storage_mask_bc( hh_storage_t s, int local_index, int flag, int owned, hh_boundary_condition_t bc, unsigned* mask );
/* ---- mesh boundary flags of the macro-vertices, -edges and -faces (SetupPrimitiveStorage.cpp:977-1090).  Default: 1 on the domain
 * boundary, 0 elsewhere.  Every rank sets the flags of the whole mesh.  The setters fail once a function, an operator or an
 * exchange plan exists on the storage.  The macro-cells share the flag of the interior and the location setters leave it alone. */
/* SetupPrimitiveStorage::setMeshBoundaryFlagsOnBoundary */
HYTEG_HOST_API int hyteg_host_storage_set_mesh_boundary_flags_on_boundary( hh_storage_t s, unsigned long long flag_on_boundary,
                                                                           unsigned long long flag_inner, int highest_dimension_always_inner );
/* SetupPrimitiveStorage::setMeshBoundaryFlagsInner */
HYTEG_HOST_API int hyteg_host_storage_set_mesh_boundary_flags_inner( hh_storage_t s, unsigned long long flag_inner, int highest_dimension_always_inner );
/* SetupPrimitiveStorage::setMeshBoundaryFlagsByVertexLocation; on_boundary( user, xyz ) != 0: the point is on that boundary */
HYTEG_HOST_API int hyteg_host_storage_set_mesh_boundary_flags_by_vertex_location( hh_storage_t s, unsigned long long flag,
                                                                                  int ( *on_boundary )( void*, const double* ), void* user,
                                                                                  int all_vertices );
/* SetupPrimitiveStorage::setMeshBoundaryFlagsByCentroidLocation (without a geometry map: cells are affine) */
HYTEG_HOST_API int hyteg_host_storage_set_mesh_boundary_flags_by_centroid_location( hh_storage_t s, unsigned long long flag,
                                                                                    int ( *on_boundary )( void*, const double* ), void* user );
/* SetupPrimitiveStorage::setMeshBoundaryFlag; dim 0: macro-vertex, 1: -edge, 2: -face, index as counted by storage_counts */
HYTEG_HOST_API int hyteg_host_storage_set_mesh_boundary_flag( hh_storage_t s, int dim, int index, unsigned long long flag );
/* Primitive::getMeshBoundaryFlag / getCoordinates, SetupPrimitiveStorage::onBoundary: the primitive's (sorted) global vertex ids,
 * their coordinates, its flag and whether it lies on the domain boundary */
HYTEG_HOST_API int hyteg_host_storage_primitive( hh_storage_t s, int dim, int index, int* nvertices, int* vertex_ids3, double* coords9,
                                                 unsigned long long* flag, int* on_boundary );
/* the exchange classes: the mesh flags 0 and 1 and every other flag present, ascending; class c has the plans of key
 * ( c & 1 ) + 2 * dof_kind + 4 * ( c >> 1 ).  flags may be NULL (count only).  No counterpart in the reference, whose
 * communication is per primitive. */
HYTEG_HOST_API int hyteg_host_storage_boundary_classes( hh_storage_t s, int* count, unsigned long long* flags );
/* a copy of the condition of functions that were given none (create0123BC, flag 1 re-typed by set_boundary_type) */
HYTEG_HOST_API int hyteg_host_storage_default_boundary_condition( hh_storage_t s, hh_boundary_condition_t* out );

/* ---- BoundaryCondition (src/hyteg/boundary/BoundaryConditions.hpp), a value: functions copy it ---- */
/* preset 0: BoundaryCondition() (every flag Inner), 1: BoundaryCondition::create0123BC, 2: BoundaryCondition::createAllInnerBC */
HYTEG_HOST_API int hyteg_host_boundary_condition_create( int preset, hh_boundary_condition_t* out );
HYTEG_HOST_API int hyteg_host_boundary_condition_destroy( hh_boundary_condition_t bc );
/* BoundaryCondition::createDomainBC (dof_type Inner: createInnerBC, Dirichlet: createDirichletBC, Neumann: createNeumannBC,
 * Freeslip: createFreeslipBC); *uid = id of the new BoundaryUID */
HYTEG_HOST_API int hyteg_host_boundary_condition_create_domain( hh_boundary_condition_t bc, const char* name, int dof_type, int nflags,
                                                                const unsigned long long* flags, int* uid );
/* BoundaryCondition::getBoundaryType */
HYTEG_HOST_API int hyteg_host_boundary_condition_type( hh_boundary_condition_t bc, unsigned long long flag, int* dof_type );
/* BoundaryCondition::getBoundaryUIDFromMeshFlag; uid 0 = the boundary of the flags that were given none */
HYTEG_HOST_API int hyteg_host_boundary_condition_uid( hh_boundary_condition_t bc, unsigned long long flag, int* uid, char* name, int buflen );
/* BoundaryCondition::operator== */
HYTEG_HOST_API int hyteg_host_boundary_condition_equal( hh_boundary_condition_t a, hh_boundary_condition_t b, int* equal );
HYTEG_HOST_API int hyteg_host_storage_set_stream( hh_storage_t s, void* stream );
/* levels <= `level` use the batched kernels (one launch for all local cells, inner and boundary points together) when the
 * rank owns more than one cell; -1 disables batching.  Default 6, or the environment variable HYTEG_AMD_BATCH_MAX_LEVEL. */
HYTEG_HOST_API int hyteg_host_storage_set_batch_max_level( hh_storage_t s, int level );
/* Stream lanes of the storage: independent interior launches inside one host-layer call (the loop of
 * hyteg_host_operator_apply_cycle: applies without shell points on different (src, dst) pairs; the cell loop of a multi-cell
 * apply when enabled) are placed on `lanes` in-order streams, lane 0 being the storage's stream, and joined before the call
 * returns; dependent launches keep the order one stream gives them.  1 = everything on the storage's stream in the order
 * of issue; 0 = the default: the environment variable HYTEG_AMD_APPLY_LANES, else 2.  At most 8.  Results do not depend on it.
 * Whatever the count, lanes are not used on a storage of several ranks, on the batched levels, while the storage's stream is
 * recorded into a graph, and while the timing tree is enabled (hyteg_host_storage_enable_timing: its ranges wait for the
 * storage's stream only) -- a run profiled with the timing tree therefore shows one-stream times. */
HYTEG_HOST_API int hyteg_host_storage_set_apply_lanes( hh_storage_t s, int lanes );
/* The cell loop of a non-batched multi-cell P1 apply: from `cells` local macro-cells on, the cells' interior kernels alternate
 * between the lanes (one fork, one join per apply).  0 = never; -1 = the default: the environment variable
 * HYTEG_AMD_APPLY_CELL_LANES_MIN, else 24 (level 8: -2.3 % on 24 cells, +7 % on 6). */
HYTEG_HOST_API int hyteg_host_storage_set_apply_cell_lanes_min( hh_storage_t s, int cells );
/* bit l of *mask: lane l carried a launch in the last lane scope of the storage (the last apply_cycle, or multi-cell apply
 * with cell lanes); 0 if the lanes were off there. */
HYTEG_HOST_API int hyteg_host_storage_lanes_seen( hh_storage_t s, unsigned* mask );
/* The planner behind it, without a GPU: step k reads the arrays read_ids[read_ptr[k] .. read_ptr[k+1]) and writes
 * write_ids[write_ptr[k] .. write_ptr[k+1]) (CSR; ids stand for device base pointers).  lane_out[k] = the lane step k is
 * issued on; bit j of waits_out[k] = before step k its lane waits for everything issued on lane j so far. */
HYTEG_HOST_API int hyteg_host_lane_plan( int lanes, int nsteps, const int* read_ptr, const unsigned long long* read_ids, const int* write_ptr,
                                         const unsigned long long* write_ids, int* lane_out, unsigned* waits_out );
/* Steps per launch of hyteg_host_operator_apply_cycle: on one rank with one local macro-cell whose shell points are all excluded,
 * consecutive steps of the cycle that are independent of each other (no step's destination array is another step's source or
 * destination) share one launch of up to `steps` applies (hyteg_hip_p1_apply_cell_steps): no kernel boundary between them.
 * 1 = one launch per apply; 0 = the default: the environment variable HYTEG_AMD_APPLY_STEPS, else 16.  At most 16.  Results do not
 * depend on it.  A group is placed on the lanes like a single apply; with several lanes a group takes at most 1 / lanes of the
 * independent steps ahead of it, so that short rings keep alternating between the lanes.  Not used on several ranks or
 * cells, on the batched levels, above level 8 (levels 2-8 only), while the stream is recorded into a graph and while the timing tree is enabled. */
HYTEG_HOST_API int hyteg_host_storage_set_apply_steps( hh_storage_t s, int steps );
/* *count: launches of more than one step that the last hyteg_host_operator_apply_cycle on this storage issued; 0 if it ran as single
 * launches (grouping off, not applicable, or no two consecutive independent steps). */
HYTEG_HOST_API int hyteg_host_storage_steps_launches( hh_storage_t s, unsigned* count );
/* The grouping behind it, without a GPU: step k = 0 .. steps-1 of a cycle over a ring of npairs pairs reads src_ids[j] and writes
 * dst_ids[j], j = ( first + k ) % npairs (ids stand for device base pointers).  sizes_out (room for `steps` entries) receives the
 * sizes of the consecutive groups, *ngroups_out their number.  lanes = 1: maximal groups of up to max_group conflict-free steps;
 * lanes > 1: a group takes 1 / lanes of the conflict-free steps ahead of it, so that every lane still gets a launch. */
HYTEG_HOST_API int hyteg_host_apply_steps_plan( int npairs, const unsigned long long* src_ids, const unsigned long long* dst_ids, int first, int steps,
                                                int max_group, int lanes, int* sizes_out, int* ngroups_out );
/* Timing tree with the reference's timer names (walberla::WcTimingTree behind PrimitiveStorage::getTimingTree():
 * "Operator P1Function to P1Function" / "Apply", "smooth_jac", "SOR"; "P1Function" / "Assign", "Dot (local)" ...;
 * "Geometric Multigrid Solver" / "Level L" / "Smoother" ...; src/hyteg/operators/Operator.hpp:148-166,
 * GeometricMultigridSolver.hpp:200-300) and its JSON dump (src/hyteg/dataexport/TimingOutput.hpp:46-60).  Off by default.
 * synchronize != 0: every range waits for the device before it stops (measures execution instead of enqueueing).
 * HYTEG_AMD_ROCTX=1 in the environment additionally emits roctx ranges with the same names.
 * timing_json: writes at most buflen bytes (NUL-terminated), *needed receives the size of the complete text. */
HYTEG_HOST_API int hyteg_host_storage_enable_timing( hh_storage_t s, int on, int synchronize );
HYTEG_HOST_API int hyteg_host_storage_timing_json( hh_storage_t s, char* buf, size_t buflen, size_t* needed );
HYTEG_HOST_API int hyteg_host_storage_timing_reset( hh_storage_t s );
/* Transport of the shared-point exchange of a storage distributed over several ranks (one process per GPU).
 * (a) RCCL over xGMI issued from the host layer itself: neighbour send/recv groups on a communication stream, ordered
 *     against the compute stream with events; all-reduce of dot products.  unique_id: HYTEG_HIP_COMM_ID_BYTES bytes from
 *     hyteg_hip_comm_unique_id on rank 0, distributed to all ranks by the application; collective over all ranks; call
 *     it with the rank's device current.  Semantics: BufferedCommunication.cpp:181-470 of the reference.
 * (b) hooks: exchange_begin( user, level, key ) starts an all-to-all of the registered send buffer of plan
 *     key = cls + 2 * dof_kind (may return before completion), exchange_end( user, level, key ) waits for it,
 *     allreduce_sum( user, values, n ) sums host values in place.  A hook returns 0 on success; any other value makes
 *     the calling operation fail (the host layer never reduces a receive buffer whose transfer failed). */
HYTEG_HOST_API int hyteg_host_storage_use_rccl( hh_storage_t s, const unsigned char* unique_id );
HYTEG_HOST_API int hyteg_host_storage_transport_name( hh_storage_t s, char* buf, int buflen );
/* (c) peer to peer on top of (a) or (b) (which keep the all-reduce and every plan that is not connected): the pack kernel
 *     stores into receive slots inside the peers' IPC-mapped arenas, a one-wave kernel waits for their sequence numbers
 *     (include/hyteg_hip.h, hyteg_hip_p2p_*) -- no library call per exchange.  Set-up, collective, any channel for the bytes:
 *       use_p2p( arena_bytes ) -> this rank's HYTEG_HIP_P2P_HANDLE_BYTES handle;  p2p_open( handles of all ranks, rank by rank );
 *       per plan: p2p_layout -> 3 byte offsets { slot 0, slot 1, flag } per peer of the plan, deliver triple k to rank
 *       peers[k];  p2p_connect( the triples the peers laid out for this rank, in the order of peers[] ).
 *     check_transport synchronises and fails if a device-side wait has timed out; drop_p2p returns to the wrapped transport. */
HYTEG_HOST_API int hyteg_host_storage_use_p2p( hh_storage_t s, size_t arena_bytes, unsigned char* handle, int* arena_kind );
HYTEG_HOST_API int hyteg_host_storage_p2p_open( hh_storage_t s, const unsigned char* handles );
HYTEG_HOST_API int hyteg_host_storage_p2p_layout( hh_storage_t s, int level, int key, long long* offsets );
HYTEG_HOST_API int hyteg_host_storage_p2p_connect( hh_storage_t s, int level, int key, const long long* offsets );
HYTEG_HOST_API int hyteg_host_storage_drop_p2p( hh_storage_t s );
HYTEG_HOST_API int hyteg_host_storage_check_transport( hh_storage_t s );
/* in-place sum over all ranks of n doubles in host memory through the storage's transport (no-op on one rank):
 * walberla::mpi::allReduceInplace( ..., SUM ) of the reference's norms and dot products */
HYTEG_HOST_API int hyteg_host_storage_allreduce_sum( hh_storage_t s, double* values, int n );
/* in-place maximum over all ranks of each of n doubles in host memory (no-op on one rank): walberla::mpi::allReduce( ..., MAX ) of
 * getMaxDoFValue and its siblings (VertexDoFFunction.cpp:1953).  Built on the transport's sum -- every rank fills its own slot of a vector
 * of zeros, in rounds of at most 16 ranks -- so it is exact and needs no further transport operation or hook.  min = -max( -x ). */
HYTEG_HOST_API int hyteg_host_storage_allreduce_max( hh_storage_t s, double* values, int n );
/* numberOfLocalDoFs / numberOfGlobalDoFs (src/hyteg/functions/FunctionTools.hpp) of a P1 function (vertex DoFs) and of a P2 function
 * (vertex + edge DoFs) at `level`, from the topology alone (no GPU); a shared DoF belongs to the rank of its lowest-numbered cell */
HYTEG_HOST_API int hyteg_host_storage_p1_number_of_dofs( hh_storage_t s, int level, int global, unsigned long long* count );
HYTEG_HOST_API int hyteg_host_storage_p2_number_of_dofs( hh_storage_t s, int level, int global, unsigned long long* count );
HYTEG_HOST_API int hyteg_host_storage_set_hooks( hh_storage_t s, int ( *exchange_begin )( void*, int, int ),
                                                 int ( *exchange_end )( void*, int, int ),
                                                 int ( *allreduce_sum )( void*, double*, int ), void* user );
/* exchange plan of (level, key = ( cls & 1 ) + 2 * dof_kind + 4 * ( cls >> 1 ), cls an index into storage_boundary_classes; dof_kind 0: vertex DoFs, 1: edge DoFs of P2 functions) -- host
 * data, works without a GPU.  sizes[0..4] = ngroups, nentries, npeers, total_send, total_recv */
HYTEG_HOST_API int hyteg_host_plan_sizes( hh_storage_t s, int level, int key, int* sizes );
HYTEG_HOST_API int hyteg_host_plan_export( hh_storage_t s, int level, int key, int* group_ptr, int* entry_buf, int* entry_off,
                                           int* peers, int* send_count, int* recv_count, int* send_buf, int* send_off );
HYTEG_HOST_API int hyteg_host_plan_register_buffers( hh_storage_t s, int level, int key, double* send_dev, double* recv_dev );

/* ---- P1Function<double> ---- */
HYTEG_HOST_API int hyteg_host_function_create( hh_storage_t s, const char* name, int min_level, int max_level, hh_function_t* out );
HYTEG_HOST_API int hyteg_host_function_destroy( hh_function_t f );
HYTEG_HOST_API int hyteg_host_function_cell_pointer( hh_function_t f, int local_cell, int level, double** dev_ptr );
HYTEG_HOST_API int hyteg_host_function_upload_cell( hh_function_t f, int local_cell, int level, const double* host );
HYTEG_HOST_API int hyteg_host_function_download_cell( hh_function_t f, int local_cell, int level, double* host );
HYTEG_HOST_API int hyteg_host_function_interpolate_constant( hh_function_t f, double value, int level, int flag );
HYTEG_HOST_API int hyteg_host_function_assign( hh_function_t dst, int n, const double* scalars, const hh_function_t* srcs, int level, int flag );
HYTEG_HOST_API int hyteg_host_function_add( hh_function_t dst, int n, const double* scalars, const hh_function_t* srcs, int level, int flag );
HYTEG_HOST_API int hyteg_host_function_mult_elementwise( hh_function_t dst, int n, const hh_function_t* srcs, int level, int flag );
HYTEG_HOST_API int hyteg_host_function_dot( hh_function_t a, hh_function_t b, int level, int flag, int global, double* result );
/* out[HYTEG_HIP_REDUCE_SUM .. HYTEG_HIP_REDUCE_MAX_ABS] = sumLocal( level, flag ), sumLocal( .., absolute ), getMinDoFValue, getMaxDoFValue,
 * getMaxDoFMagnitude of the function (VertexDoFFunction.cpp:1796-2057) from ONE pass over its arrays; mpi_reduce != 0: reduced over the
 * ranks (sumGlobal; mpiReduce = true).  The extrema always include the cell interiors, as in the reference (see P1Function::reduceLocal). */
HYTEG_HOST_API int hyteg_host_p1_reduce( hh_function_t f, int level, int flag, int mpi_reduce, double* out );
HYTEG_HOST_API int hyteg_host_function_sum_shared( hh_function_t f, int level, int flag );
HYTEG_HOST_API int hyteg_host_function_sync_shared( hh_function_t f, int level, int flag );
/* BoundaryCondition::createAllInnerBC() for this function (the pressure of a Stokes function): every point counts as Inner */
HYTEG_HOST_API int hyteg_host_function_set_all_inner( hh_function_t f, int on );
/* Function::setBoundaryCondition / getBoundaryCondition (the latter a copy, to be destroyed by the caller) */
HYTEG_HOST_API int hyteg_host_function_set_boundary_condition( hh_function_t f, hh_boundary_condition_t bc );
HYTEG_HOST_API int hyteg_host_function_boundary_condition( hh_function_t f, hh_boundary_condition_t* out );
/* Function::interpolate( constant, level, BoundaryUID ): on the primitives whose mesh flag belongs to that boundary of the
 * function's condition.  Id and name as hyteg_host_boundary_condition_create_domain / _uid gave them: a uid of another condition fails */
HYTEG_HOST_API int hyteg_host_function_interpolate_constant_on_boundary( hh_function_t f, double value, int level, int boundary_uid,
                                                                         const char* boundary_name );

/* ---- P1ConstantOperator< Form > (src/constant_stencil_operator/P1ConstantOperator.hpp:165-210)
 * form 0: Laplace, 1: mass, 2-4: P1Div{x,y,z}Operator, 5-7: P1DivT{x,y,z}Operator, 8: P1PSPGOperator ---- */
HYTEG_HOST_API int hyteg_host_operator_create( hh_storage_t s, int min_level, int max_level, int form, hh_operator_t* out );
HYTEG_HOST_API int hyteg_host_operator_destroy( hh_operator_t op );
/* inner[15], slots[14*15] of a GLOBAL cell id */
HYTEG_HOST_API int hyteg_host_operator_stencils( hh_operator_t op, int global_cell, int level, double* inner15, double* slots210 );
HYTEG_HOST_API int hyteg_host_operator_apply( hh_operator_t op, hh_function_t src, hh_function_t dst, int level, int flag, int update );
/* `steps` consecutive applies cycling over `npairs` (src, dst) function pairs: step k uses pair (first + k) % npairs.
 * The loop a C++ application would write around Operator::apply (apps/benchmarks/ApplyBenchmark/ApplyBenchmark.cpp:95-101);
 * lets a non-C++ driver time K applies without paying its own per-call overhead K times. */
HYTEG_HOST_API int hyteg_host_operator_apply_cycle( hh_operator_t op, int npairs, const hh_function_t* srcs, const hh_function_t* dsts,
                                                    int level, int flag, int update, int first, int steps );
/* the same loop between two timing events of the C-ABI (hyteg_hip_event_create_timing; NULL = none), recorded on the storage's
 * stream directly before the first and after the last apply: the device time of exactly these `steps` applies */
HYTEG_HOST_API int hyteg_host_operator_apply_cycle_timed( hh_operator_t op, int npairs, const hh_function_t* srcs, const hh_function_t* dsts,
                                                          int level, int flag, int update, int first, int steps, void* ev_start, void* ev_stop );
HYTEG_HOST_API int hyteg_host_operator_smooth_jac( hh_operator_t op, hh_function_t dst, hh_function_t rhs, hh_function_t src, double relax, int level, int flag );
HYTEG_HOST_API int hyteg_host_operator_smooth_sor( hh_operator_t op, hh_function_t dst, hh_function_t rhs, double relax, int level, int flag, int backwards );
/* one sweep of `n` functions by shared launches where the batched kernels apply (P1ConstantOperator::smooth_sor_many): the
 * same bits as n calls of hyteg_host_operator_smooth_sor */
HYTEG_HOST_API int hyteg_host_operator_smooth_sor_many( hh_operator_t op, int n, const hh_function_t* dsts, const hh_function_t* rhss, double relax,
                                                        int level, int flag, int backwards );
HYTEG_HOST_API int hyteg_host_operator_compute_inverse_diagonal( hh_operator_t op );
HYTEG_HOST_API int hyteg_host_operator_inverse_diagonal( hh_operator_t op, hh_function_t* out /* borrowed */ );

/* hyteg::operatorgeneration::P1ElementwiseDiffusion (module hyteg_operators; sample class
 * apps/2023-zikeli-mt/MT-apps/operators-used/P1ElementwiseDiffusion_cubes_const_float64.hpp:64-93): apply() hands every
 * macro-cell's arrays, vertex coordinates and micro_edges_per_macro_edge to the C-ABI seam
 * hyteg_hip_p1_elementwise_diffusion_apply_macro_3d_masked; computeInverseDiagonalOperatorValues / getInverseDiagonalValues;
 * smooth_jac as P1ElementwiseOperator.cpp:288-331 */
HYTEG_HOST_API int hyteg_host_elementwise_create( hh_storage_t s, int min_level, int max_level, hh_elementwise_t* out );
HYTEG_HOST_API int hyteg_host_elementwise_destroy( hh_elementwise_t op );
HYTEG_HOST_API int hyteg_host_elementwise_apply( hh_elementwise_t op, hh_function_t src, hh_function_t dst, int level, int flag, int update );
HYTEG_HOST_API int hyteg_host_elementwise_compute_inverse_diagonal( hh_elementwise_t op );
HYTEG_HOST_API int hyteg_host_elementwise_inverse_diagonal( hh_elementwise_t op, hh_function_t* out /* borrowed */ );
HYTEG_HOST_API int hyteg_host_elementwise_smooth_jac( hh_elementwise_t op, hh_function_t dst, hh_function_t rhs, hh_function_t src, double relax,
                                                      int level, int flag );

/* hyteg::operatorgeneration::P1ElementwiseDivKGrad( storage, minLevel, maxLevel, k ) (module hyteg_operators; call site
 * tests/hyteg/convergence/ElementwiseDivKGradCGConvergenceTest.cpp:73-81): -div( k grad u ) with a P1 coefficient function that
 * holds values on every level min_level..max_level (levels 0..8).  The handle shares ownership of k.  apply / inverse diagonal /
 * smooth_jac as for the class above; smooth_jac is one fused launch on the inner points unless set_fused( 0 ) selects the four
 * composed passes of P1ElementwiseOperator.cpp:288-331 everywhere.  residual: r = b - A x as a multigrid cycle forms it
 * (GeometricMultigridSolver.hpp:240-246), one fused launch on the inner points as well; set_fused( 0 ) also composes the residual
 * and the steps of the Chebyshev smoother. */
typedef void* hh_divkgrad_t;
typedef void* hh_divkgrad_solver_t;
HYTEG_HOST_API int hyteg_host_divkgrad_create( hh_storage_t s, int min_level, int max_level, hh_function_t k, hh_divkgrad_t* out );
HYTEG_HOST_API int hyteg_host_divkgrad_destroy( hh_divkgrad_t op );
HYTEG_HOST_API int hyteg_host_divkgrad_apply( hh_divkgrad_t op, hh_function_t src, hh_function_t dst, int level, int flag, int update );
HYTEG_HOST_API int hyteg_host_divkgrad_compute_inverse_diagonal( hh_divkgrad_t op );
HYTEG_HOST_API int hyteg_host_divkgrad_inverse_diagonal( hh_divkgrad_t op, hh_function_t* out /* borrowed */ );
HYTEG_HOST_API int hyteg_host_divkgrad_smooth_jac( hh_divkgrad_t op, hh_function_t dst, hh_function_t rhs, hh_function_t src, double relax, int level,
                                                   int flag );
HYTEG_HOST_API int hyteg_host_divkgrad_residual( hh_divkgrad_t op, hh_function_t x, hh_function_t b, hh_function_t r, int level, int flag );
HYTEG_HOST_API int hyteg_host_divkgrad_set_fused( hh_divkgrad_t op, int on );
/* Solvers for this operator type: CGSolver (preconditioner: any solver of this group, or null), GeometricMultigridSolver with the
 * linear P1 transfer, a CG coarse-grid solver and WeightedJacobiSmoother( relax ) or ChebyshevSmoother (fused steps; radii: one
 * spectral radius, or one per level) as its smoother, the two smoothers on their own (smoother: 0 weighted Jacobi, -1 identity),
 * and chebyshev::estimateRadius (ChebyshevSmoother.hpp:655-666). */
HYTEG_HOST_API int hyteg_host_divkgrad_cg_create( hh_storage_t s, int min_level, int max_level, int max_iter, double tol,
                                                  hh_divkgrad_solver_t preconditioner /* or null */, hh_divkgrad_solver_t* out );
HYTEG_HOST_API int hyteg_host_divkgrad_cg_iterations( hh_divkgrad_solver_t solver, int* iterations );
HYTEG_HOST_API int hyteg_host_divkgrad_smoother_create( hh_storage_t s, int min_level, int max_level, int smoother, double relax,
                                                        hh_divkgrad_solver_t* out );
HYTEG_HOST_API int hyteg_host_divkgrad_gmg_create( hh_storage_t s, int min_level, int max_level, double relax, int pre, int post, int wcycle,
                                                   int cg_max_iter, double cg_tol, hh_divkgrad_solver_t* out );
HYTEG_HOST_API int hyteg_host_divkgrad_chebyshev_estimate_radius( hh_divkgrad_t op, int level, int max_iter, hh_function_t x, hh_function_t tmp,
                                                                  double* radius );
HYTEG_HOST_API int hyteg_host_divkgrad_chebyshev_create( hh_storage_t s, int min_level, int max_level, int order, const double* radii, int n_radii,
                                                         double upper, double lower, hh_divkgrad_solver_t* out );
HYTEG_HOST_API int hyteg_host_divkgrad_gmg_create_chebyshev( hh_storage_t s, int min_level, int max_level, int order, const double* radii, int n_radii,
                                                             double upper, double lower, int pre, int post, int wcycle, int cg_max_iter,
                                                             double cg_tol, hh_divkgrad_solver_t* out );
HYTEG_HOST_API int hyteg_host_divkgrad_solver_solve( hh_divkgrad_solver_t solver, hh_divkgrad_t op, hh_function_t x, hh_function_t b, int level );
HYTEG_HOST_API int hyteg_host_divkgrad_solver_destroy( hh_divkgrad_solver_t solver );

/* hyteg::P1ElementwiseAffineEpsilonOperator( storage, minLevel, maxLevel, viscosity ) (src/mixed_operator/P1EpsilonOperator.hpp:
 * 89-164): -div( 2 mu eps(u) ) on a P1VectorFunction, here given as its three component functions (src / dst / rhs: arrays of three
 * handles, e.g. the velocity components of a Stokes function).  The reference's viscosity is a std::function sampled at the points
 * of a degree-2 rule; here mu is a P1 function that holds values on every level min_level..max_level (levels 0..8): the same
 * operator where mu is linear per micro-cell.  The handle shares ownership of mu.  Every component is masked by its own boundary
 * condition.  inverse_diagonal: three borrowed handles (the diagonals of the diagonal blocks, extractInverseDiagonal); smooth_jac
 * is one fused launch on the inner points unless set_fused( 0 ) selects the composed passes of P1ElementwiseOperator.cpp:288-331.
 * residual: r = b - A x as a multigrid cycle forms it (GeometricMultigridSolver.hpp:240-246), one fused launch on the inner points
 * as well; set_fused( 0 ) also composes the residual and the steps of the Chebyshev smoother. */
typedef void* hh_epsilon_t;
typedef void* hh_epsilon_solver_t;
typedef void* hh_epsilon_stokes_t;
typedef void* hh_epsilon_stokes_solver_t;
HYTEG_HOST_API int hyteg_host_epsilon_create( hh_storage_t s, int min_level, int max_level, hh_function_t mu, hh_epsilon_t* out );
HYTEG_HOST_API int hyteg_host_epsilon_destroy( hh_epsilon_t op );
HYTEG_HOST_API int hyteg_host_epsilon_apply( hh_epsilon_t op, const hh_function_t* src /* 3 */, const hh_function_t* dst /* 3 */, int level, int flag,
                                             int update );
HYTEG_HOST_API int hyteg_host_epsilon_compute_inverse_diagonal( hh_epsilon_t op );
HYTEG_HOST_API int hyteg_host_epsilon_inverse_diagonal( hh_epsilon_t op, hh_function_t* out /* 3, borrowed */ );
HYTEG_HOST_API int hyteg_host_epsilon_smooth_jac( hh_epsilon_t op, const hh_function_t* dst, const hh_function_t* rhs, const hh_function_t* src,
                                                  double relax, int level, int flag );
HYTEG_HOST_API int hyteg_host_epsilon_set_fused( hh_epsilon_t op, int on );
HYTEG_HOST_API int hyteg_host_epsilon_residual( hh_epsilon_t op, const hh_function_t* x, const hh_function_t* b, const hh_function_t* r, int level,
                                                int flag );
/* Solvers for this operator type, acting on three component functions (x, b: arrays of three handles): CGSolver (preconditioner: any
 * solver of this group, or null), GeometricMultigridSolver with the linear P1 transfer on every component
 * (P1VectorFunctionLinearRestriction / Prolongation), a CG coarse-grid solver and WeightedJacobiSmoother( relax ) or ChebyshevSmoother
 * (fused steps; radii: one spectral radius, or one per level) as its smoother, the smoothers on their own (smoother: 0 weighted
 * Jacobi, -1 identity), and chebyshev::estimateRadius (ChebyshevSmoother.hpp:655-666) from a fixed start vector. */
HYTEG_HOST_API int hyteg_host_epsilon_chebyshev_estimate_radius( hh_epsilon_t op, int level, int max_iter, double* radius );
HYTEG_HOST_API int hyteg_host_epsilon_cg_create( hh_storage_t s, int min_level, int max_level, int max_iter, double tol,
                                                 hh_epsilon_solver_t preconditioner /* or null */, hh_epsilon_solver_t* out );
HYTEG_HOST_API int hyteg_host_epsilon_cg_iterations( hh_epsilon_solver_t solver, int* iterations );
HYTEG_HOST_API int hyteg_host_epsilon_smoother_create( hh_storage_t s, int min_level, int max_level, int smoother, double relax,
                                                       hh_epsilon_solver_t* out );
HYTEG_HOST_API int hyteg_host_epsilon_gmg_create( hh_storage_t s, int min_level, int max_level, double relax, int pre, int post, int wcycle,
                                                  int cg_max_iter, double cg_tol, hh_epsilon_solver_t* out );
HYTEG_HOST_API int hyteg_host_epsilon_chebyshev_create( hh_storage_t s, int min_level, int max_level, int order, const double* radii, int n_radii,
                                                        double upper, double lower, hh_epsilon_solver_t* out );
HYTEG_HOST_API int hyteg_host_epsilon_gmg_create_chebyshev( hh_storage_t s, int min_level, int max_level, int order, const double* radii, int n_radii,
                                                            double upper, double lower, int pre, int post, int wcycle, int cg_max_iter,
                                                            double cg_tol, hh_epsilon_solver_t* out );
HYTEG_HOST_API int hyteg_host_epsilon_solver_solve( hh_epsilon_solver_t solver, hh_epsilon_t op, const hh_function_t* x, const hh_function_t* b,
                                                    int level );
HYTEG_HOST_API int hyteg_host_epsilon_solver_destroy( hh_epsilon_solver_t solver );
/* hyteg::P1P1ElementwiseAffineEpsilonStokesOperator( storage, minLevel, maxLevel, viscosity )
 * (src/mixed_operator/P1P1ElementwiseAffineEpsilonStokesOperator.hpp:32-92) on P1 Stokes functions: the operator above on the
 * velocity, the constant-stencil div / divT blocks and the PSPG block.  MinResSolver for it: preconditioner 0 identity, 1
 * StokesPressureBlockPreconditioner< ., P1LumpedInvMassOperator > (solvertemplates::stokesMinResSolver,
 * src/hyteg/solvers/solvertemplates/StokesSolverTemplates.hpp:54-69), 2 the same with the pressure action
 * x.p = mu .* invLumpedMass .* b.p (mu: the viscosity function; null for 0 and 1).  minres_precondition applies the solver's
 * preconditioner on its own: x = M^-1 b.
 * minres_create_block: MinResSolver with StokesVectorBlockDiagonalPreconditioner -- velocity_cycles multigrid V-cycles on the epsilon
 * operator as the velocity action (smoother 0 weighted Jacobi( relax ), 1 Chebyshev( order ) with radii: none (n_radii 0) = estimated
 * per level at construction, one, or one per level; pre = post smoothing steps; CG on the coarsest level), the lumped inverse mass on
 * the pressure, weighted with mu if viscosity_weighted.  mu: the viscosity of the operator the solver is used with.  The action has
 * to be symmetric positive definite: any other smoother, pre != post or velocity_cycles < 1 are errors. */
HYTEG_HOST_API int hyteg_host_epsilon_stokes_create( hh_storage_t s, int min_level, int max_level, hh_function_t mu, hh_epsilon_stokes_t* out );
HYTEG_HOST_API int hyteg_host_epsilon_stokes_destroy( hh_epsilon_stokes_t op );
HYTEG_HOST_API int hyteg_host_epsilon_stokes_apply( hh_epsilon_stokes_t op, hh_stokes_function_t src, hh_stokes_function_t dst, int level, int flag );
HYTEG_HOST_API int hyteg_host_epsilon_stokes_minres_create( hh_storage_t s, int min_level, int max_level, int max_iter, double rel_tol,
                                                            int preconditioner, hh_function_t mu /* or null */, hh_epsilon_stokes_solver_t* out );
HYTEG_HOST_API int hyteg_host_epsilon_stokes_minres_create_block( hh_storage_t s, int min_level, int max_level, int max_iter, double rel_tol,
                                                                  int viscosity_weighted, hh_function_t mu, int velocity_cycles, int smoother, int order,
                                                                  const double* radii /* or null */, int n_radii, double relax, int pre, int post,
                                                                  int cg_max_iter, double cg_tol, hh_epsilon_stokes_solver_t* out );
HYTEG_HOST_API int hyteg_host_epsilon_stokes_minres_solve( hh_epsilon_stokes_solver_t solver, hh_epsilon_stokes_t op, hh_stokes_function_t x,
                                                           hh_stokes_function_t b, int level );
HYTEG_HOST_API int hyteg_host_epsilon_stokes_minres_precondition( hh_epsilon_stokes_solver_t solver, hh_epsilon_stokes_t op, hh_stokes_function_t x,
                                                                  hh_stokes_function_t b, int level );
HYTEG_HOST_API int hyteg_host_epsilon_stokes_minres_iterations( hh_epsilon_stokes_solver_t solver, int* iterations );
HYTEG_HOST_API int hyteg_host_epsilon_stokes_minres_destroy( hh_epsilon_stokes_solver_t solver );

/* ---- grid transfer ---- */
HYTEG_HOST_API int hyteg_host_restrict( hh_function_t f, int source_level, int flag );
HYTEG_HOST_API int hyteg_host_prolongate( hh_function_t f, int source_level, int flag );
HYTEG_HOST_API int hyteg_host_prolongate_and_add( hh_function_t f, int source_level, int flag );
/* P1toP2Conversion( p1, p2, P2Level, flag ) / P2toP1Conversion( p2, p1, P1Level, flag )
 * (src/hyteg/gridtransferoperators/P1toP2Conversion.cpp:28-149, P2toP1Conversion.cpp:28-150): the P2 function of level L and the P1
 * function of level L + 1 have the same DoFs; the values `flag` selects are copied, one launch per chunk of macro-cells.  The
 * levels follow the reference: the first call takes the P2 level, the second the P1 level.  The flag is translated with the
 * source function's boundary condition; no exchange follows. */
HYTEG_HOST_API int hyteg_host_p1_to_p2( hh_function_t p1, hh_p2function_t p2, int p2_level, int flag );
HYTEG_HOST_API int hyteg_host_p2_to_p1( hh_p2function_t p2, hh_function_t p1, int p1_level, int flag );
/* P1toP1QuadraticProlongationThroughP2Injection( storage, p1MinLevel, p1MaxLevel )
 * (src/hyteg/gridtransferoperators/P1toP1QuadraticProlongationThroughP2Injection.hpp:33-55): prolongate( f, source_level, flag ) =
 * P1toP2Conversion( All ), P2toP2QuadraticProlongation::prolongate( flag ), P2toP1Conversion( All ) through a P2 function the
 * object owns.  1 <= p1_min_level (the reference asks for > 2), source_level in p1_min_level .. p1_max_level - 1 and
 * p1_max_level <= 10.  The DoFs of level source_level + 1 that `flag` excludes are overwritten with zero: restore boundary
 * values afterwards. */
typedef void* hh_quadratic_prolongation_t;
HYTEG_HOST_API int hyteg_host_quadratic_prolongation_create( hh_storage_t s, int p1_min_level, int p1_max_level, hh_quadratic_prolongation_t* out );
HYTEG_HOST_API int hyteg_host_quadratic_prolongation_prolongate( hh_quadratic_prolongation_t p, hh_function_t f, int source_level, int flag );
HYTEG_HOST_API int hyteg_host_quadratic_prolongation_destroy( hh_quadratic_prolongation_t p );

/* ---- solvers on the Laplace operator ----
 * smoother: 0 = weighted Jacobi (relax), 1 = Gauss-Seidel, 2 = SOR (relax), 3 = mixed-precision Jacobi (relax), 5 = symmetric
 * Gauss-Seidel, 6 = symmetric SOR (relax): SymmetricGaussSeidelSmoother / SymmetricSORSmoother (SymmetricSORSmoother.hpp:29-65), a forward
 * sweep followed by a backward one.  Coarse grid: CG. */
HYTEG_HOST_API int hyteg_host_gmg_create( hh_storage_t s, int min_level, int max_level, int smoother, double relax, int pre, int post,
                                          int wcycle, int cg_max_iter, double cg_tol, hh_solver_t* out );
/* ---- ChebyshevSmoother (replaces src/hyteg/solvers/ChebyshevSmoother.hpp:40-555 at its call sites) ----
 * coefficients: replaces setupCoefficientsInternal (ChebyshevSmoother.hpp:329-552) for any order 1..8: out[0 .. order-1] are the
 *   monomial coefficients of p in 1 - l p( l ) = T_n( ( theta - l ) / delta ) / T_n( theta / delta ), theta = ( upper + lower ) / 2,
 *   delta = ( upper - lower ) / 2.  Touches no GPU.
 * estimate_radius: replaces chebyshev::estimateRadius (ChebyshevSmoother.hpp:655-666; power iteration of
 *   src/hyteg/numerictools/SpectrumEstimation.hpp:56-84 on D^-1 A, flag All).  x: start vector (overwritten), tmp: work function;
 *   needs compute_inverse_diagonal.
 * create: a ChebyshevSmoother of the given order for hyteg_host_solver_solve; radii: one spectral radius of D^-1 A for all levels
 *   (n_radii = 1) or one per level min_level..max_level; bounds upper * radius and lower * radius (the reference's defaults: 1.2, 0.3;
 *   setupCoefficients, ChebyshevSmoother.hpp:243-316).  The operator needs compute_inverse_diagonal before the first solve.
 * set_fused: ChebyshevSmoother::setFused of the smoother itself or of a multigrid solver's smoother (default on: one launch per
 *   step on the cell interiors; off: apply + multElementwise + assign).
 * gmg_create_chebyshev: hyteg_host_gmg_create with that smoother (pre / post = smoother calls per level). */
HYTEG_HOST_API int hyteg_host_chebyshev_coefficients( int order, double lower, double upper, double* out /* order */ );
HYTEG_HOST_API int hyteg_host_chebyshev_estimate_radius( hh_operator_t op, int level, int max_iter, hh_function_t x, hh_function_t tmp,
                                                         double* radius );
HYTEG_HOST_API int hyteg_host_chebyshev_create( hh_storage_t s, int min_level, int max_level, int order, const double* radii, int n_radii,
                                                double upper, double lower, hh_solver_t* out );
HYTEG_HOST_API int hyteg_host_chebyshev_set_fused( hh_solver_t solver, int on );
HYTEG_HOST_API int hyteg_host_gmg_create_chebyshev( hh_storage_t s, int min_level, int max_level, int order, const double* radii, int n_radii,
                                                    double upper, double lower, int pre, int post, int wcycle, int cg_max_iter, double cg_tol,
                                                    hh_solver_t* out );
/* launch graphs of the cycle (hyteg_host.hpp, GeometricMultigridSolver::setUseGraphs): opt-in, storages of one rank;
 * replayed_cycles counts the cycles that ran from a recording */
HYTEG_HOST_API int hyteg_host_gmg_set_use_graphs( hh_solver_t solver, int on );
HYTEG_HOST_API int hyteg_host_gmg_replayed_cycles( hh_solver_t solver, int* count );
/* FullMultigridSolver (src/hyteg/solvers/FullMultigridSolver.hpp:33-114) around a multigrid solver of hyteg_host_gmg_create /
 * _gmg_create_chebyshev, which it shares (the multigrid solver's handle may be destroyed before this one).
 * solve( level ), through hyteg_host_solver_solve: for l = min_level .. level: cycles_per_level[l] cycles on level l,
 * post_cycle( l, user ), the prolongation of x from l to l + 1 with the flag Inner | NeumannBoundary | FreeslipBoundary if
 * l < max_level, post_prolongate( l, user ) -- also on the top level.  cycles_per_level: n_cycles = 0: cycles_per_level[0] cycles on
 * every level; otherwise one count per level 0 .. max_level (those below min_level are ignored), any other number is an error.
 * prolongation: 0 = P1toP1LinearProlongation, 1 = P1toP1QuadraticProlongationThroughP2Injection (min_level >= 1, max_level <= 10).
 * The callbacks may be null. */
typedef void ( *hh_level_callback_t )( uint64_t level, void* user );
HYTEG_HOST_API int hyteg_host_fmg_create( hh_storage_t s, hh_solver_t gmg, int min_level, int max_level, const unsigned* cycles_per_level, int n_cycles,
                                          int prolongation, hh_level_callback_t post_cycle, void* post_cycle_user,
                                          hh_level_callback_t post_prolongate, void* post_prolongate_user, hh_solver_t* out );
/* CGSolver::setUseDeviceScalars / setUseSingleLaunch (hyteg_host.hpp); on: bit 0 = alpha, beta and the convergence test stay
 * on the device (storages of one rank up to level 5), bit 1 = problems that fit one workgroup are solved by one launch
 * (both default on); `solver` is a CG solver or a multigrid solver whose coarse solver is one */
HYTEG_HOST_API int hyteg_host_cg_set_use_device_scalars( hh_solver_t solver, int on );
/* CGSolver::getIterations of the last solve */
HYTEG_HOST_API int hyteg_host_cg_iterations( hh_solver_t solver, int* iterations );
HYTEG_HOST_API int hyteg_host_cg_create( hh_storage_t s, int min_level, int max_level, int max_iter, double tol, hh_solver_t* out );
/* CGSolver with a preconditioner (CGSolver.hpp:44-63, eighth constructor argument): any solver handle -- a multigrid solver, a smoother
 * of hyteg_host_smoother_create, a Chebyshev smoother.  The CG solver shares ownership of the preconditioner, so its handle may be
 * destroyed first.  The loop is the reference's (init() :340-358, iteration :146-201); on P1 functions the update of x and r and the
 * reduction <r,r> are one pass (hyteg_hip_p1_cg_update_cells), which set_use_fused_update( 0 ) replaces by the three composed calls. */
HYTEG_HOST_API int hyteg_host_cg_create_preconditioned( hh_storage_t s, int min_level, int max_level, int max_iter, double tol,
                                                        hh_solver_t preconditioner, hh_solver_t* out );
HYTEG_HOST_API int hyteg_host_cg_set_use_fused_update( hh_solver_t solver, int on );
/* a smoother on its own, for hyteg_host_solver_solve or as a preconditioner: the codes of hyteg_host_gmg_create, and -1 =
 * IdentityPreconditioner (x = b) */
HYTEG_HOST_API int hyteg_host_smoother_create( hh_storage_t s, int min_level, int max_level, int smoother, double relax, hh_solver_t* out );
HYTEG_HOST_API int hyteg_host_solver_solve( hh_solver_t solver, hh_operator_t laplace, hh_function_t x, hh_function_t b, int level );
/* Solver::solveSteps (Solver.hpp): `steps` calls of solve, which a smoother may fuse -- what GeometricMultigridSolver calls for its
 * pre- and post-smoothing */
HYTEG_HOST_API int hyteg_host_solver_solve_steps( hh_solver_t solver, hh_operator_t laplace, hh_function_t x, hh_function_t b, int level, int steps );
/* MixedPrecisionJacobiSmoother( storage, minLevel, maxLevel, relax, fp32Sweeps ) on its own (hyteg_amd/host/solvers.hpp; no class of
 * the reference: its pieces are the float instantiation of the generated kernels and VertexDoFFunction::copyFrom); inside a
 * multigrid solver it is smoother 3 of hyteg_host_gmg_create */
HYTEG_HOST_API int hyteg_host_mixed_precision_jacobi_create( hh_storage_t s, int min_level, int max_level, double relax, int fp32_sweeps,
                                                             hh_solver_t* out );
HYTEG_HOST_API int hyteg_host_solver_destroy( hh_solver_t solver );

/* ---- P1-P1 Stokes: P1StokesFunction (composites/P1StokesFunction.hpp: velocity with the storage's boundary types, pressure
 * with createAllInnerBC), P1P1StokesOperator::apply (mixed_operator/P1P1StokesOperator.hpp:51-64), UzawaSmoother
 * (solvers/UzawaSmoother.hpp:262-288) over StokesVelocityBlockBlockDiagonalPreconditioner, geometric multigrid with
 * P1P1StokesToP1P1Stokes{Restriction,Prolongation} and a dense direct coarse-grid solver standing in for PETScLUSolver ---- */
HYTEG_HOST_API int hyteg_host_stokes_function_create( hh_storage_t s, const char* name, int min_level, int max_level, hh_stokes_function_t* out );
HYTEG_HOST_API int hyteg_host_stokes_function_destroy( hh_stokes_function_t f );
/* k = 0, 1, 2: velocity components, 3: pressure; the handle is a view owned by the Stokes function (do not destroy it) */
HYTEG_HOST_API int hyteg_host_stokes_function_component( hh_stokes_function_t f, int k, hh_function_t* out );
HYTEG_HOST_API int hyteg_host_stokes_function_assign( hh_stokes_function_t dst, int n, const double* scalars, const hh_stokes_function_t* fs, int level, int flag );
HYTEG_HOST_API int hyteg_host_stokes_function_dot( hh_stokes_function_t a, hh_stokes_function_t b, int level, int flag, double* out );
/* vertexdof::projectMean (VertexDoFFunction.hpp:586-592) */
HYTEG_HOST_API int hyteg_host_project_mean( hh_function_t pressure, int level );
HYTEG_HOST_API int hyteg_host_stokes_operator_create( hh_storage_t s, int min_level, int max_level, hh_stokes_operator_t* out );
HYTEG_HOST_API int hyteg_host_stokes_operator_destroy( hh_stokes_operator_t op );
HYTEG_HOST_API int hyteg_host_stokes_operator_apply( hh_stokes_operator_t op, hh_stokes_function_t src, hh_stokes_function_t dst, int level, int flag );
/* velocity_smoother: 0 weighted Jacobi, 1 Gauss-Seidel, 2 SOR (relaxation velocity_relax) on every velocity component */
HYTEG_HOST_API int hyteg_host_stokes_uzawa_create( hh_storage_t s, int min_level, int max_level, double relax, int velocity_iterations,
                                                   int velocity_smoother, double velocity_relax, hh_stokes_solver_t* out );
HYTEG_HOST_API int hyteg_host_stokes_gmg_create( hh_storage_t s, hh_stokes_solver_t smoother, int min_level, int max_level, int pre, int post,
                                                 int increment, int project_mean_after_restriction, hh_stokes_solver_t* out );
/* GeometricMultigridSolver< P1P1StokesOperator > with a choice of coarse-grid solver: 0 = dense LU on the host (stand-in for
 * PETScLUSolver, single rank), 1 = MinResSolver preconditioned with StokesPressureBlockPreconditioner< P1P1StokesOperator,
 * P1LumpedInvMassOperator > (apps/stokesSphere/StokesSphere.cpp:227-237; any number of ranks) */
HYTEG_HOST_API int hyteg_host_stokes_gmg_create_with_coarse( hh_storage_t s, hh_stokes_solver_t smoother, int min_level, int max_level, int pre, int post,
                                                             int increment, int project_mean_after_restriction, int coarse, int coarse_max_iter,
                                                             double coarse_rel_tol, hh_stokes_solver_t* out );
/* MinResSolver< P1P1StokesOperator > (src/hyteg/solvers/MinresSolver.hpp): preconditioner 0 identity, 1 pressure block (lumped
 * inverse mass), 2 StokesBlockDiagonalPreconditioner with `velocity_steps` V(2,2) Laplace cycles per velocity component */
HYTEG_HOST_API int hyteg_host_stokes_minres_create( hh_storage_t s, int min_level, int max_level, int max_iter, double rel_tol, int preconditioner,
                                                    int velocity_steps, hh_stokes_solver_t* out );
HYTEG_HOST_API int hyteg_host_stokes_minres_iterations( hh_stokes_solver_t solver, int* iterations );
/* MinResSolver< P1ConstantLaplaceOperator > with JacobiPreconditioner( jacobi_iterations ) (0: identity) */
HYTEG_HOST_API int hyteg_host_solver_create_minres( hh_storage_t s, int min_level, int max_level, int max_iter, double rel_tol, int jacobi_iterations,
                                                    hh_solver_t* out );
HYTEG_HOST_API int hyteg_host_stokes_solver_solve( hh_stokes_solver_t solver, hh_stokes_operator_t op, hh_stokes_function_t x, hh_stokes_function_t b, int level );
HYTEG_HOST_API int hyteg_host_stokes_solver_destroy( hh_stokes_solver_t solver );

/* ---- P2Function / P2ElementwiseLaplaceOperator (first version): any number of macro-cells on ONE rank ----
 * vertex part: the P1 cell array; edge part: hyteg_hip_p2_edge_array_size( level ) doubles (EdgeDoFIndexing.hpp:920-985) */
HYTEG_HOST_API int hyteg_host_p2function_create( hh_storage_t s, const char* name, int min_level, int max_level, hh_p2function_t* out );
HYTEG_HOST_API int hyteg_host_p2function_destroy( hh_p2function_t f );
HYTEG_HOST_API int hyteg_host_p2function_pointers( hh_p2function_t f, int local_cell, int level, double** vertex_dev, double** edge_dev );
HYTEG_HOST_API int hyteg_host_p2function_upload( hh_p2function_t f, int local_cell, int level, const double* vertex_host, const double* edge_host );
HYTEG_HOST_API int hyteg_host_p2function_download( hh_p2function_t f, int local_cell, int level, double* vertex_host, double* edge_host );
HYTEG_HOST_API int hyteg_host_p2function_interpolate_constant( hh_p2function_t f, double value, int level, int flag );
/* P2Function::setBoundaryCondition (vertex- and edge-DoF part) / getBoundaryCondition / interpolate( constant, level, BoundaryUID ) */
HYTEG_HOST_API int hyteg_host_p2function_set_boundary_condition( hh_p2function_t f, hh_boundary_condition_t bc );
HYTEG_HOST_API int hyteg_host_p2function_boundary_condition( hh_p2function_t f, hh_boundary_condition_t* out );
HYTEG_HOST_API int hyteg_host_p2function_interpolate_constant_on_boundary( hh_p2function_t f, double value, int level, int boundary_uid,
                                                                           const char* boundary_name );
HYTEG_HOST_API int hyteg_host_p2function_assign( hh_p2function_t dst, int n, const double* scalars, const hh_p2function_t* srcs, int level, int flag );
HYTEG_HOST_API int hyteg_host_p2function_add( hh_p2function_t dst, int n, const double* scalars, const hh_p2function_t* srcs, int level, int flag );
/* P2Function::multElementwise (src/hyteg/p2functionspace/P2Function.cpp: vertex- and edge-DoF parts separately) */
HYTEG_HOST_API int hyteg_host_p2function_mult_elementwise( hh_p2function_t dst, int n, const hh_p2function_t* srcs, int level, int flag );
HYTEG_HOST_API int hyteg_host_p2function_dot( hh_p2function_t a, hh_p2function_t b, int level, int flag, double* result );
/* hyteg_host_p1_reduce for a P2 function: vertex-DoF and edge-DoF parts combined as in P2Function.cpp:351-365, :566-605 */
HYTEG_HOST_API int hyteg_host_p2_reduce( hh_p2function_t f, int level, int flag, int mpi_reduce, double* out );
HYTEG_HOST_API int hyteg_host_p2operator_create( hh_storage_t s, int min_level, int max_level, hh_p2operator_t* out );
/* P2toP2QuadraticProlongation::prolongate / prolongateAndAdd (add != 0) from source_level to source_level + 1 and
 * P2toP2QuadraticRestriction::restrict from source_level to source_level - 1 (src/hyteg/gridtransferoperators/) */
HYTEG_HOST_API int hyteg_host_p2_prolongate( hh_p2function_t f, int source_level, int flag, int add );
HYTEG_HOST_API int hyteg_host_p2_restrict( hh_p2function_t f, int source_level, int flag );
/* P2ConstantLaplaceOperator (src/constant_stencil_operator/P2ConstantOperator.hpp): same handle type and calls as the
 * elementwise operator; on affine macro-cells the assembled constant stencils ARE what the kernel's operator table holds */
HYTEG_HOST_API int hyteg_host_p2operator_create_constant( hh_storage_t s, int min_level, int max_level, hh_p2operator_t* out );
/* the inner-DoF stencils a P2ConstantLaplaceOperator assembled for a local cell (levels >= 2): the values of the four maps
 * v2v | e2v | v2e | e2e in the order of hyteg_hip_p2_constant_stencil_layout */
HYTEG_HOST_API int hyteg_host_p2operator_constant_stencils( hh_p2operator_t op, int local_cell, int level, double* out, int capacity, int* count );
HYTEG_HOST_API int hyteg_host_p2operator_destroy( hh_p2operator_t op );
/* the six 10 x 10 element matrices (FEniCS ordering) of a local cell at `level` */
HYTEG_HOST_API int hyteg_host_p2operator_element_matrices( hh_p2operator_t op, int local_cell, int level, double* out600 );
HYTEG_HOST_API int hyteg_host_p2operator_apply( hh_p2operator_t op, hh_p2function_t src, hh_p2function_t dst, int level, int flag, int update );
/* P2 Jacobi smoother and multigrid.  compute_inverse_diagonal: P2ElementwiseOperator::computeInverseDiagonalOperatorValues
 * (P2ElementwiseOperator.hpp:110, .cpp:420-520); smooth_jac: .cpp:344-374 (dst != src);  gmg: GeometricMultigridSolver
 * (src/hyteg/solvers/GeometricMultigridSolver.hpp) over WeightedJacobiSmoother, P2toP2QuadraticRestriction / Prolongation and a CG
 * coarse-grid solver -- the composition of tests/hyteg/P2/P2GMG3DConvergenceTest.cpp with the Jacobi smoother in place of its
 * Gauss-Seidel one (the edge-DoF Gauss-Seidel kernels are not built). */
typedef void* hh_p2solver_t;
HYTEG_HOST_API int hyteg_host_p2operator_compute_inverse_diagonal( hh_p2operator_t op );
HYTEG_HOST_API int hyteg_host_p2operator_inverse_diagonal_copy( hh_p2operator_t op, hh_p2function_t dst, int level );
HYTEG_HOST_API int hyteg_host_p2operator_smooth_jac( hh_p2operator_t op, hh_p2function_t dst, hh_p2function_t rhs, hh_p2function_t src, double relax,
                                                     int level, int flag );
/* smooth_sor: P2ConstantOperator::smooth_sor (P2ConstantOperator.cpp:113-153; macro-cell part :913-1200: vertex DoFs in
 * lexicographic order, then the edge DoFs type by type; backwards: reversed).  Exactly the reference's sweep inside a macro-cell;
 * on DoFs shared between macro-cells a different Gauss-Seidel ordering of the same splitting.  Needs
 * compute_inverse_diagonal.  gmg smoother: 0 weighted Jacobi( relax ), 1 Gauss-Seidel, 2 SOR( relax ), 5 symmetric Gauss-Seidel,
 * 6 symmetric SOR( relax ) (a forward sweep, then a backward one). */
HYTEG_HOST_API int hyteg_host_p2operator_smooth_sor( hh_p2operator_t op, hh_p2function_t dst, hh_p2function_t rhs, double relax, int level, int flag,
                                                     int backwards );
HYTEG_HOST_API int hyteg_host_p2_gmg_create( hh_storage_t s, int min_level, int max_level, int smoother, double relax, int pre, int post, int wcycle,
                                             int cg_max_iter, double cg_tol, hh_p2solver_t* out );
/* ChebyshevSmoother< P2ElementwiseLaplaceOperator > (ChebyshevSmoother.hpp:40-555; the generic sequence apply, multElementwise,
 * assign) on its own, its radius estimate (ChebyshevSmoother.hpp:655-666) and as the smoother of the multigrid solver above;
 * arguments as for the P1 entries hyteg_host_chebyshev_create / _estimate_radius / hyteg_host_gmg_create_chebyshev */
HYTEG_HOST_API int hyteg_host_p2_chebyshev_estimate_radius( hh_p2operator_t op, int level, int max_iter, hh_p2function_t x, hh_p2function_t tmp,
                                                            double* radius );
HYTEG_HOST_API int hyteg_host_p2_chebyshev_create( hh_storage_t s, int min_level, int max_level, int order, const double* radii, int n_radii,
                                                   double upper, double lower, hh_p2solver_t* out );
HYTEG_HOST_API int hyteg_host_p2_gmg_create_chebyshev( hh_storage_t s, int min_level, int max_level, int order, const double* radii, int n_radii,
                                                       double upper, double lower, int pre, int post, int wcycle, int cg_max_iter, double cg_tol,
                                                       hh_p2solver_t* out );
/* hyteg_host_fmg_create for a P2 multigrid solver of the entries above; the FMG prolongation is P2toP2QuadraticProlongation */
HYTEG_HOST_API int hyteg_host_p2_fmg_create( hh_storage_t s, hh_p2solver_t gmg, int min_level, int max_level, const unsigned* cycles_per_level,
                                             int n_cycles, hh_level_callback_t post_cycle, void* post_cycle_user,
                                             hh_level_callback_t post_prolongate, void* post_prolongate_user, hh_p2solver_t* out );
HYTEG_HOST_API int hyteg_host_p2_solver_solve( hh_p2solver_t solver, hh_p2operator_t op, hh_p2function_t x, hh_p2function_t b, int level );
HYTEG_HOST_API int hyteg_host_p2_solver_destroy( hh_p2solver_t solver );
/* the P2 twins of hyteg_host_cg_create_preconditioned, hyteg_host_cg_iterations and hyteg_host_smoother_create (codes 0, 1, 2, 5, 6, -1) */
HYTEG_HOST_API int hyteg_host_p2_cg_create_preconditioned( hh_storage_t s, int min_level, int max_level, int max_iter, double tol,
                                                           hh_p2solver_t preconditioner, hh_p2solver_t* out );
HYTEG_HOST_API int hyteg_host_p2_cg_iterations( hh_p2solver_t solver, int* iterations );
HYTEG_HOST_API int hyteg_host_p2_smoother_create( hh_storage_t s, int min_level, int max_level, int smoother, double relax, hh_p2solver_t* out );
/* CGSolver< P2ElementwiseLaplaceOperator > on one level, flags Inner | NeumannBoundary as in the reference's CGSolver */
HYTEG_HOST_API int hyteg_host_p2_cg_solve( hh_storage_t s, hh_p2operator_t op, hh_p2function_t x, hh_p2function_t b, int level, int max_iter,
                                           double tol, int* iterations );

/* ---- P2ElementwiseDivKGrad: -div( k grad u ) on P2 with a P2 coefficient (hyteg_amd/host/p2divkgrad.hpp) ----
 * operatorgeneration::P2ElementwiseDivKGrad( storage, minLevel, maxLevel, const P2Function< real_t >& k ) of module hyteg_operators
 * (tests/hyteg/convergence/ElementwiseDivKGradCGConvergenceTest.cpp:192-221) with the interface of P2ElementwiseOperator -- apply, gemv,
 * computeInverseDiagonalOperatorValues, smooth_jac -- and the solver templates instantiated for it as they are: CGSolver (with a
 * preconditioner or without), WeightedJacobiSmoother / IdentityPreconditioner (smoother 0 / -1), ChebyshevSmoother,
 * GeometricMultigridSolver< ., P2toP2QuadraticRestriction, P2toP2QuadraticProlongation > with CG on the coarsest level, and
 * FullMultigridSolver around it.  The handle keeps k alive; the operator at level l reads k at level l.  Levels 0..8.
 * P2ElementwiseMassOperator = P2ElementwiseOperator< forms::P2MassForm > (P2ElementwiseOperator.hpp): the right-hand side of that test. */
typedef void* hh_p2divkgrad_t;
typedef void* hh_p2divkgrad_solver_t;
typedef void* hh_p2massoperator_t;
HYTEG_HOST_API int hyteg_host_p2divkgrad_create( hh_storage_t s, int min_level, int max_level, hh_p2function_t k, hh_p2divkgrad_t* out );
HYTEG_HOST_API int hyteg_host_p2divkgrad_destroy( hh_p2divkgrad_t op );
HYTEG_HOST_API int hyteg_host_p2divkgrad_apply( hh_p2divkgrad_t op, hh_p2function_t src, hh_p2function_t dst, int level, int flag, int update );
HYTEG_HOST_API int hyteg_host_p2divkgrad_gemv( hh_p2divkgrad_t op, double alpha, hh_p2function_t src, double beta, hh_p2function_t dst, int level,
                                               int flag );
HYTEG_HOST_API int hyteg_host_p2divkgrad_compute_inverse_diagonal( hh_p2divkgrad_t op );
HYTEG_HOST_API int hyteg_host_p2divkgrad_inverse_diagonal_copy( hh_p2divkgrad_t op, hh_p2function_t dst, int level );
HYTEG_HOST_API int hyteg_host_p2divkgrad_smooth_jac( hh_p2divkgrad_t op, hh_p2function_t dst, hh_p2function_t rhs, hh_p2function_t src, double relax,
                                                     int level, int flag );
/* setFused: the fused residual / Jacobi / Chebyshev entries of the operator (default on), or the composed passes; residual: r = b - A x
 * as a multigrid cycle writes it (GeometricMultigridSolver.hpp:240-246) */
HYTEG_HOST_API int hyteg_host_p2divkgrad_set_fused( hh_p2divkgrad_t op, int on );
HYTEG_HOST_API int hyteg_host_p2divkgrad_chebyshev_fusable( hh_p2divkgrad_t op, int level, int* fusable ); /* chebyshevFusable( level ) */
HYTEG_HOST_API int hyteg_host_p2divkgrad_residual( hh_p2divkgrad_t op, hh_p2function_t x, hh_p2function_t b, hh_p2function_t r, int level, int flag );
HYTEG_HOST_API int hyteg_host_p2divkgrad_cg_create( hh_storage_t s, int min_level, int max_level, int max_iter, double tol,
                                                    hh_p2divkgrad_solver_t preconditioner /* or null */, hh_p2divkgrad_solver_t* out );
HYTEG_HOST_API int hyteg_host_p2divkgrad_cg_iterations( hh_p2divkgrad_solver_t solver, int* iterations );
HYTEG_HOST_API int hyteg_host_p2divkgrad_smoother_create( hh_storage_t s, int min_level, int max_level, int smoother, double relax,
                                                          hh_p2divkgrad_solver_t* out );
HYTEG_HOST_API int hyteg_host_p2divkgrad_gmg_create( hh_storage_t s, int min_level, int max_level, double relax, int pre, int post, int wcycle,
                                                     int cg_max_iter, double cg_tol, hh_p2divkgrad_solver_t* out );
HYTEG_HOST_API int hyteg_host_p2divkgrad_chebyshev_estimate_radius( hh_p2divkgrad_t op, int level, int max_iter, hh_p2function_t x, hh_p2function_t tmp,
                                                                    double* radius );
HYTEG_HOST_API int hyteg_host_p2divkgrad_chebyshev_create( hh_storage_t s, int min_level, int max_level, int order, const double* radii, int n_radii,
                                                           double upper, double lower, hh_p2divkgrad_solver_t* out );
HYTEG_HOST_API int hyteg_host_p2divkgrad_gmg_create_chebyshev( hh_storage_t s, int min_level, int max_level, int order, const double* radii, int n_radii,
                                                               double upper, double lower, int pre, int post, int wcycle, int cg_max_iter,
                                                               double cg_tol, hh_p2divkgrad_solver_t* out );
HYTEG_HOST_API int hyteg_host_p2divkgrad_fmg_create( hh_storage_t s, hh_p2divkgrad_solver_t gmg, int min_level, int max_level,
                                                     const unsigned* cycles_per_level, int n_cycles, hh_p2divkgrad_solver_t* out );
HYTEG_HOST_API int hyteg_host_p2divkgrad_solver_solve( hh_p2divkgrad_solver_t solver, hh_p2divkgrad_t op, hh_p2function_t x, hh_p2function_t b,
                                                       int level );
HYTEG_HOST_API int hyteg_host_p2divkgrad_solver_destroy( hh_p2divkgrad_solver_t solver );
HYTEG_HOST_API int hyteg_host_p2massoperator_create( hh_storage_t s, int min_level, int max_level, hh_p2massoperator_t* out );
HYTEG_HOST_API int hyteg_host_p2massoperator_apply( hh_p2massoperator_t op, hh_p2function_t src, hh_p2function_t dst, int level, int flag, int update );
HYTEG_HOST_API int hyteg_host_p2massoperator_destroy( hh_p2massoperator_t op );

/* ---- P2-P1 Taylor-Hood Stokes (BASELINE config 5's "P2-P1 Stokes block operator"; hyteg_amd/host/taylorhood.hpp) ----
 * P2P1TaylorHoodFunction (composites/P2P1TaylorHoodFunction.hpp): three P2 velocity components + a P1 pressure (all-inner boundary
 * condition); P2P1TaylorHoodStokesOperator::apply (mixed_operator/P2P1TaylorHoodStokesOperator.hpp:55-64): Laplace on the velocity,
 * divT (P1 -> P2) added, div (P2 -> P1) into the pressure.  The handles returned by _velocity / _pressure are views that live as
 * long as the Taylor-Hood function.  gmg: the composition of tests/hyteg/convergence/P2P1Stokes3DUzawaConvergenceTest.cpp:150-163
 * (Uzawa over Gauss-Seidel, quadratic / linear transfer, projectMean after the restriction) with pressure-preconditioned MINRES on the
 * coarsest level in place of PETSc's LU. */
typedef void* hh_th_function_t;
typedef void* hh_th_operator_t;
typedef void* hh_th_solver_t;
HYTEG_HOST_API int hyteg_host_th_function_create( hh_storage_t s, const char* name, int min_level, int max_level, hh_th_function_t* out );
HYTEG_HOST_API int hyteg_host_th_function_destroy( hh_th_function_t f );
HYTEG_HOST_API int hyteg_host_th_function_velocity( hh_th_function_t f, int k, hh_p2function_t* out );
HYTEG_HOST_API int hyteg_host_th_function_pressure( hh_th_function_t f, hh_function_t* out );
HYTEG_HOST_API int hyteg_host_th_function_assign( hh_th_function_t dst, int n, const double* scalars, const hh_th_function_t* fs, int level, int flag );
HYTEG_HOST_API int hyteg_host_th_function_interpolate_constant( hh_th_function_t f, double value, int level, int flag );
HYTEG_HOST_API int hyteg_host_th_function_dot( hh_th_function_t a, hh_th_function_t b, int level, int flag, double* out );
HYTEG_HOST_API int hyteg_host_th_operator_create( hh_storage_t s, int min_level, int max_level, hh_th_operator_t* out );
HYTEG_HOST_API int hyteg_host_th_operator_destroy( hh_th_operator_t op );
HYTEG_HOST_API int hyteg_host_th_operator_apply( hh_th_operator_t op, hh_th_function_t src, hh_th_function_t dst, int level, int flag );
/* which: 0 div (velocity of src -> pressure of dst), 1 divT (pressure of src -> velocity of dst) */
HYTEG_HOST_API int hyteg_host_th_operator_apply_block( hh_th_operator_t op, int which, hh_th_function_t src, hh_th_function_t dst, int level, int flag );
HYTEG_HOST_API int hyteg_host_th_gmg_create( hh_storage_t s, int min_level, int max_level, double uzawa_relax, int pre, int post, int increment,
                                             int coarse_max_iter, double coarse_rel_tol, hh_th_solver_t* out );
HYTEG_HOST_API int hyteg_host_th_minres_create( hh_storage_t s, int min_level, int max_level, int max_iter, double rel_tol, hh_th_solver_t* out );
HYTEG_HOST_API int hyteg_host_th_solver_solve( hh_th_solver_t solver, hh_th_operator_t op, hh_th_function_t x, hh_th_function_t b, int level );
HYTEG_HOST_API int hyteg_host_th_solver_destroy( hh_th_solver_t solver );
HYTEG_HOST_API int hyteg_host_th_project_pressure_mean( hh_th_function_t f, int level );
/* the 10 x 10 element matrix (FEniCS ordering) of a mixed block as the P2 kernel gets it: which 0 = div (p2_to_p1_tet_div_tet, edge rows
 * zero), 1 = divT (p1_to_p2_tet_divt_tet, edge columns zero); component k; coords[4][3] */
HYTEG_HOST_API int hyteg_host_th_form_element_matrix( int which, int k, const double* coords12, double* out100 );

/* ---- variable-viscosity Taylor-Hood Stokes (hyteg_amd/host/p2epsilon.hpp) ----
 * operatorgeneration::P2ViscousBlockEpsilonOperator( storage, minLevel, maxLevel, const P2Function< real_t >& mu ): -div( 2 mu eps( u ) ) on
 * a P2VectorFunction (three hh_p2function_t, each with its own boundary condition) with a P2 viscosity that the caller interpolates on
 * every level used -- apply, gemv, computeInverseDiagonalOperatorValues (the inverse diagonals of the three diagonal blocks; the
 * returned handles are views owned by the operator handle), smooth_jac -- and the solver templates instantiated for it as they are:
 * CGSolver (with a preconditioner or without), WeightedJacobiSmoother / IdentityPreconditioner (smoother 0 / -1), ChebyshevSmoother.
 * operatorgeneration::P2P1StokesEpsilonOperator( storage, minLevel, maxLevel, mu ) on P2P1TaylorHoodFunction: viscOp Replace, divT Add,
 * div Replace (src/mixed_operator/P2P1ElementwiseAffineEpsilonStokesOperator.hpp:61-70), and MinResSolver on it; preconditioner
 * 0 identity, 1 StokesPressureBlockPreconditioner< ., P1LumpedInvMassOperator > (solvertemplates::stokesMinResSolver; the P2 half of
 * tests/hyteg/convergence/ElementwiseEpsilonMinResConvergenceTest.cpp:366-412), 2 the same with the pressure action weighted with mu at
 * the vertex DoFs (mu: the viscosity, needed for 2 only).  The handles keep mu alive.  Levels 0..8. */
typedef void* hh_p2epsilon_t;
typedef void* hh_p2epsilon_solver_t;
typedef void* hh_th_epsilon_t;
typedef void* hh_th_epsilon_solver_t;
HYTEG_HOST_API int hyteg_host_p2epsilon_create( hh_storage_t s, int min_level, int max_level, hh_p2function_t mu, hh_p2epsilon_t* out );
HYTEG_HOST_API int hyteg_host_p2epsilon_destroy( hh_p2epsilon_t op );
HYTEG_HOST_API int hyteg_host_p2epsilon_apply( hh_p2epsilon_t op, const hh_p2function_t* src /* 3 */, const hh_p2function_t* dst /* 3 */, int level,
                                               int flag, int update );
HYTEG_HOST_API int hyteg_host_p2epsilon_gemv( hh_p2epsilon_t op, double alpha, const hh_p2function_t* src, double beta, const hh_p2function_t* dst,
                                              int level, int flag );
HYTEG_HOST_API int hyteg_host_p2epsilon_compute_inverse_diagonal( hh_p2epsilon_t op );
HYTEG_HOST_API int hyteg_host_p2epsilon_inverse_diagonal( hh_p2epsilon_t op, hh_p2function_t* out /* 3 */ );
HYTEG_HOST_API int hyteg_host_p2epsilon_smooth_jac( hh_p2epsilon_t op, const hh_p2function_t* dst, const hh_p2function_t* rhs, const hh_p2function_t* src,
                                                    double relax, int level, int flag );
/* setFused: the fused residual / Jacobi / Chebyshev entries of the operator (default on), or the composed passes; residual: r = b - A x
 * as a multigrid cycle writes it (GeometricMultigridSolver.hpp:240-246), on three component functions each */
HYTEG_HOST_API int hyteg_host_p2epsilon_set_fused( hh_p2epsilon_t op, int on );
HYTEG_HOST_API int hyteg_host_p2epsilon_chebyshev_fusable( hh_p2epsilon_t op, int level, int* fusable ); /* chebyshevFusable( level ) */
HYTEG_HOST_API int hyteg_host_p2epsilon_residual( hh_p2epsilon_t op, const hh_p2function_t* x, const hh_p2function_t* b, const hh_p2function_t* r,
                                                  int level, int flag );
/* GeometricMultigridSolver on the operator with the quadratic P2 transfer on every component (P2toP2QuadraticVectorRestriction /
 * Prolongation), a CG coarse-grid solver and WeightedJacobiSmoother( relax ) or ChebyshevSmoother (fused steps; radii: one spectral
 * radius, or one per level) as its smoother */
HYTEG_HOST_API int hyteg_host_p2epsilon_gmg_create( hh_storage_t s, int min_level, int max_level, double relax, int pre, int post, int wcycle,
                                                    int cg_max_iter, double cg_tol, hh_p2epsilon_solver_t* out );
HYTEG_HOST_API int hyteg_host_p2epsilon_gmg_create_chebyshev( hh_storage_t s, int min_level, int max_level, int order, const double* radii, int n_radii,
                                                              double upper, double lower, int pre, int post, int wcycle, int cg_max_iter,
                                                              double cg_tol, hh_p2epsilon_solver_t* out );
HYTEG_HOST_API int hyteg_host_p2epsilon_cg_create( hh_storage_t s, int min_level, int max_level, int max_iter, double tol,
                                                   hh_p2epsilon_solver_t preconditioner /* or null */, hh_p2epsilon_solver_t* out );
HYTEG_HOST_API int hyteg_host_p2epsilon_cg_iterations( hh_p2epsilon_solver_t solver, int* iterations );
HYTEG_HOST_API int hyteg_host_p2epsilon_smoother_create( hh_storage_t s, int min_level, int max_level, int smoother, double relax,
                                                         hh_p2epsilon_solver_t* out );
HYTEG_HOST_API int hyteg_host_p2epsilon_chebyshev_estimate_radius( hh_p2epsilon_t op, int level, int max_iter, double* radius );
HYTEG_HOST_API int hyteg_host_p2epsilon_chebyshev_create( hh_storage_t s, int min_level, int max_level, int order, const double* radii, int n_radii,
                                                          double upper, double lower, hh_p2epsilon_solver_t* out );
HYTEG_HOST_API int hyteg_host_p2epsilon_solver_solve( hh_p2epsilon_solver_t solver, hh_p2epsilon_t op, const hh_p2function_t* x, const hh_p2function_t* b,
                                                      int level );
HYTEG_HOST_API int hyteg_host_p2epsilon_solver_destroy( hh_p2epsilon_solver_t solver );
HYTEG_HOST_API int hyteg_host_th_epsilon_create( hh_storage_t s, int min_level, int max_level, hh_p2function_t mu, hh_th_epsilon_t* out );
HYTEG_HOST_API int hyteg_host_th_epsilon_destroy( hh_th_epsilon_t op );
HYTEG_HOST_API int hyteg_host_th_epsilon_apply( hh_th_epsilon_t op, hh_th_function_t src, hh_th_function_t dst, int level, int flag );
HYTEG_HOST_API int hyteg_host_th_epsilon_minres_create( hh_storage_t s, int min_level, int max_level, int max_iter, double rel_tol, int preconditioner,
                                                        hh_p2function_t mu /* or null */, hh_th_epsilon_solver_t* out );
/* MinResSolver with StokesVectorBlockDiagonalPreconditioner: velocity_cycles multigrid V-cycles on the P2 epsilon operator on the levels
 * velocity_min_level .. max_level (smoother 0 weighted Jacobi( relax ), 1 Chebyshev( order; radii null: estimated per level at
 * construction ), pre = post steps, CG on the coarsest level) and the lumped inverse pressure mass, weighted with mu at the vertex DoFs if
 * viscosity_weighted.  The action has to be symmetric positive definite: any other smoother, pre != post or velocity_cycles < 1 are
 * errors.  The velocity operator's inverse diagonals are assembled on first use. */
HYTEG_HOST_API int hyteg_host_th_epsilon_minres_create_block( hh_storage_t s, int min_level, int max_level, int max_iter, double rel_tol,
                                                              int viscosity_weighted, hh_p2function_t mu, int velocity_min_level, int velocity_cycles,
                                                              int smoother, int order, const double* radii /* or null */, int n_radii, double relax,
                                                              int pre, int post, int cg_max_iter, double cg_tol, hh_th_epsilon_solver_t* out );
HYTEG_HOST_API int hyteg_host_th_epsilon_minres_solve( hh_th_epsilon_solver_t solver, hh_th_epsilon_t op, hh_th_function_t x, hh_th_function_t b,
                                                       int level );
/* x = P b: the preconditioner of the solver alone (tests restate MINRES around it) */
HYTEG_HOST_API int hyteg_host_th_epsilon_minres_precondition( hh_th_epsilon_solver_t solver, hh_th_epsilon_t op, hh_th_function_t x, hh_th_function_t b,
                                                              int level );
HYTEG_HOST_API int hyteg_host_th_epsilon_minres_iterations( hh_th_epsilon_solver_t solver, int* iterations );
HYTEG_HOST_API int hyteg_host_th_epsilon_minres_destroy( hh_th_epsilon_solver_t solver );

/* ---- strong free-slip boundaries (src/hyteg/p1functionspace/P1ProjectNormalOperator.hpp,
 * src/hyteg/composites/StrongFreeSlipWrapper.hpp) ----
 * hyteg_host_project_normal_create: P1ProjectNormalOperator( storage, minLevel, maxLevel, normal_function ).  normal( user, xyz, n )
 * writes the (not necessarily unit) normal at xyz and returns 0; another value fails the call.  It is evaluated once, in this call,
 * at the vertex DoFs of the macro-faces with one neighbour cell and of their edges and vertices, on every level -- the points
 * hyteg_host_storage_shell_points returns -- and nowhere else. */
typedef void* hh_project_normal_t;
typedef void* hh_freeslip_wrapper_t;
typedef void* hh_freeslip_solver_t;
typedef int ( *hh_normal_callback_t )( void* user, const double* xyz, double* normal );
/* entries of the shell enumeration of a macro-cell, 4 tri( 2^level + 1 ) (hyteg_hip_p1_shell_enumeration) */
HYTEG_HOST_API int hyteg_host_storage_shell_size( int level, int* out );
/* xyz[3 q + r]: coordinates of entry q of the shell enumeration of local cell li where the normal function is evaluated, NaN
 * where it is not (skipped entries, primitives inside the domain).  Host only: touches no device. */
HYTEG_HOST_API int hyteg_host_storage_shell_points( hh_storage_t s, int local_cell, int level, double* xyz );
HYTEG_HOST_API int hyteg_host_project_normal_create( hh_storage_t s, int min_level, int max_level, hh_normal_callback_t normal, void* user,
                                                     hh_project_normal_t* out );
HYTEG_HOST_API int hyteg_host_project_normal_destroy( hh_project_normal_t p );
/* project( u, v, w, level, flag ) and project( P1StokesFunction, level, flag ): ( u, v, w ) -= ( ( u, v, w ) . n ) n on the primitives
 * `flag` selects under the boundary condition of u; fails if that takes a macro-face between two cells */
HYTEG_HOST_API int hyteg_host_project_normal_project( hh_project_normal_t p, hh_function_t u, hh_function_t v, hh_function_t w, int level, int flag );
HYTEG_HOST_API int hyteg_host_project_normal_project_stokes( hh_project_normal_t p, hh_stokes_function_t f, int level, int flag );
/* StrongFreeSlipWrapper< P1P1StokesOperator, P1ProjectNormalOperator, pre_projection >( op, projection, flag ); apply is Replace only */
HYTEG_HOST_API int hyteg_host_stokes_freeslip_wrapper_create( hh_stokes_operator_t op, hh_project_normal_t p, int flag, int pre_projection,
                                                              hh_freeslip_wrapper_t* out );
HYTEG_HOST_API int hyteg_host_stokes_freeslip_wrapper_destroy( hh_freeslip_wrapper_t w );
HYTEG_HOST_API int hyteg_host_stokes_freeslip_wrapper_apply( hh_freeslip_wrapper_t w, hh_stokes_function_t src, hh_stokes_function_t dst, int level,
                                                             int flag );
/* MinResSolver< StrongFreeSlipWrapper< ... > >; preconditioner 0 identity, 1 pressure block; 2 (block diagonal) is refused: it does
 * not keep projected velocities projected.  solve() needs a wrapper with the same pre_projection. */
HYTEG_HOST_API int hyteg_host_stokes_freeslip_minres_create( hh_storage_t s, int min_level, int max_level, int max_iter, double rel_tol,
                                                             int preconditioner, int pre_projection, hh_freeslip_solver_t* out );
HYTEG_HOST_API int hyteg_host_stokes_freeslip_minres_solve( hh_freeslip_solver_t solver, hh_freeslip_wrapper_t w, hh_stokes_function_t x,
                                                            hh_stokes_function_t b, int level );
HYTEG_HOST_API int hyteg_host_stokes_freeslip_minres_iterations( hh_freeslip_solver_t solver, int* iterations );
HYTEG_HOST_API int hyteg_host_stokes_freeslip_minres_destroy( hh_freeslip_solver_t solver );
/* The same for P2 velocities and the Taylor-Hood operator: P2ProjectNormalOperator (src/hyteg/p2functionspace/P2ProjectNormalOperator.hpp)
 * is the vertex projection on the vertex-DoF parts plus the projection on the edge-DoF parts, whose normals are evaluated at the
 * midpoints of the micro-edges -- the points hyteg_host_storage_edge_shell_points returns in the order of
 * hyteg_hip_p2_edge_shell_enumeration (NaN where the function is not evaluated; host only). */
typedef void* hh_p2_project_normal_t;
HYTEG_HOST_API int hyteg_host_storage_edge_shell_size( int level, int* out );
HYTEG_HOST_API int hyteg_host_storage_edge_shell_points( hh_storage_t s, int local_cell, int level, double* xyz );
HYTEG_HOST_API int hyteg_host_p2_project_normal_create( hh_storage_t s, int min_level, int max_level, hh_normal_callback_t normal, void* user,
                                                        hh_p2_project_normal_t* out );
HYTEG_HOST_API int hyteg_host_p2_project_normal_destroy( hh_p2_project_normal_t p );
HYTEG_HOST_API int hyteg_host_p2_project_normal_project( hh_p2_project_normal_t p, hh_p2function_t u, hh_p2function_t v, hh_p2function_t w, int level,
                                                         int flag );
HYTEG_HOST_API int hyteg_host_p2_project_normal_project_stokes( hh_p2_project_normal_t p, hh_th_function_t f, int level, int flag );
/* StrongFreeSlipWrapper< P2P1TaylorHoodStokesOperator, P2ProjectNormalOperator, pre_projection > and its MINRES solver */
HYTEG_HOST_API int hyteg_host_th_freeslip_wrapper_create( hh_th_operator_t op, hh_p2_project_normal_t p, int flag, int pre_projection,
                                                          hh_freeslip_wrapper_t* out );
HYTEG_HOST_API int hyteg_host_th_freeslip_wrapper_destroy( hh_freeslip_wrapper_t w );
HYTEG_HOST_API int hyteg_host_th_freeslip_wrapper_apply( hh_freeslip_wrapper_t w, hh_th_function_t src, hh_th_function_t dst, int level, int flag );
HYTEG_HOST_API int hyteg_host_th_freeslip_minres_create( hh_storage_t s, int min_level, int max_level, int max_iter, double rel_tol,
                                                         int preconditioner, int pre_projection, hh_freeslip_solver_t* out );
HYTEG_HOST_API int hyteg_host_th_freeslip_minres_solve( hh_freeslip_solver_t solver, hh_freeslip_wrapper_t w, hh_th_function_t x, hh_th_function_t b,
                                                        int level );
HYTEG_HOST_API int hyteg_host_th_freeslip_minres_iterations( hh_freeslip_solver_t solver, int* iterations );
HYTEG_HOST_API int hyteg_host_th_freeslip_minres_destroy( hh_freeslip_solver_t solver );

#ifdef __cplusplus
}
#endif
#endif
