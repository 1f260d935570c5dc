/*
 * hyteg_hip.h -- C-ABI of libhyteg_hip.so: MI355X (gfx950) kernels for HyTeG's matrix-free P1
 * hot path (constant-stencil apply, smoothers, vector kernels, grid transfer on macro-cells).
 *
 * This is the drop-in boundary.  HyTeG has no plugin/FFI mechanism; the seam is the set of free
 * functions in namespace hyteg::vertexdof::macrocell::generated that P1ConstantOperator and
 * VertexDoFFunction call with raw pointers.  Each entry point below names
 * the reference function (file:line under /root/reference/) it replaces.  INTEGRATION.md shows the
 * binding a HyTeG maintainer would add on the reference side.
 *
 * Conventions
 *  - plain C, no C++/torch types.  All array pointers are DEVICE pointers (hipMalloc'ed or any
 *    pointer valid on the current HIP device, e.g. a torch tensor's data_ptr()).
 *  - arrays use HyTeG's linear tetrahedral macro-cell layout
 *    (src/hyteg/indexing/MacroCellIndexing.hpp:40-52): width = 2^level + 1, x fastest, then y,
 *    then z; size = width (width+1) (width+2) / 6.
 *  - stencil weights w[15] are passed BY VALUE from host memory in the iteration order of the
 *    reference's std::map<indexing::Index, real_t> (sorted by z, then y, then x;
 *    src/hyteg/indexing/Common.hpp:67-71):
 *       0:( 0, 0,-1)  1:( 1, 0,-1)  2:(-1, 1,-1)  3:( 0, 1,-1)
 *       4:( 0,-1, 0)  5:( 1,-1, 0)  6:(-1, 0, 0)  7:( 0, 0, 0)  8:( 1, 0, 0)  9:(-1, 1, 0) 10:( 0, 1, 0)
 *      11:( 0,-1, 1) 12:( 1,-1, 1) 13:(-1, 0, 1) 14:( 0, 0, 1)
 *    so a binding fills it with   for (auto& e : stencilMap) w[k++] = e.second;
 *  - neighbour-cell counts nnc[14] = { edge0..5, face0..3, vertex0..3 }, the argument order of the
 *    reference's grid-transfer kernels.
 *  - every kernel launch is asynchronous on `stream` (a hipStream_t passed as void*; NULL = the
 *    legacy default stream) and stream-ordered with respect to other work on that stream.
 *  - return value: HYTEG_HIP_OK or an error code; hyteg_hip_last_error() gives a message.
 *    The reference aborts the process on failure (WALBERLA_ABORT); a binding should do the same.
 *  - fp64 only, like the reference's generated 3-D kernels (non-double aborts there:
 *    src/constant_stencil_operator/P1ConstantOperator.cpp:417-420).
 *  - levels 2..11 (int32 indexing, as in the reference's generated kernels).  The operator loops
 *    in the reference only run for level >= 2 (src/hyteg/p1functionspace/P1Operator.hpp:293).
 */
#ifndef HYTEG_HIP_H
#define HYTEG_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#if defined( HYTEG_HIP_BUILDING )
#define HYTEG_HIP_API __attribute__( ( visibility( "default" ) ) )
#else
#define HYTEG_HIP_API
#endif

enum
{
   HYTEG_HIP_OK      = 0,
   HYTEG_HIP_EINVAL  = 1, /* bad argument (null pointer, level out of range, aliasing src==dst ...) */
   HYTEG_HIP_ELAUNCH = 2, /* HIP runtime reported an error for a launch / memcpy */
   HYTEG_HIP_ENOMEM  = 3,
   HYTEG_HIP_ENODEV  = 4, /* no usable gfx950 device */
   HYTEG_HIP_ENOTSUP = 5  /* valid arguments, but this entry point has no kernel for them: the caller takes its other path */
};

/* UpdateType, src/hyteg/types/types.hpp:29-33 */
enum
{
   HYTEG_HIP_REPLACE = 0,
   HYTEG_HIP_ADD     = 1
};

#define HYTEG_HIP_MIN_LEVEL 2
#define HYTEG_HIP_MAX_LEVEL 11
#define HYTEG_HIP_MAX_SRCS 4 /* assign/add/mult take at most this many source functions */

typedef void* hyteg_hip_stream_t;

/* ---- runtime -------------------------------------------------------------------------------- */
HYTEG_HIP_API const char* hyteg_hip_version( void );
HYTEG_HIP_API const char* hyteg_hip_last_error( void );
HYTEG_HIP_API int         hyteg_hip_device_count( int* count );
HYTEG_HIP_API int         hyteg_hip_set_device( int device );
/* name + gcnArchName of the current device, e.g. "AMD Instinct MI355X (gfx950:sramecc+:xnack-)" */
HYTEG_HIP_API int hyteg_hip_device_name( char* buf, size_t buflen );

/* device memory standing in for FunctionMemory<double>'s per-level std::vector
 * (src/hyteg/memory/FunctionMemory.hpp:109-113,216) */
HYTEG_HIP_API int hyteg_hip_malloc( void** dev_ptr, size_t bytes );
HYTEG_HIP_API int hyteg_hip_free( void* dev_ptr );
HYTEG_HIP_API int hyteg_hip_memset_zero( void* dev_ptr, size_t bytes, hyteg_hip_stream_t stream );
HYTEG_HIP_API int hyteg_hip_upload( void* dev_dst, const void* host_src, size_t bytes, hyteg_hip_stream_t stream );
HYTEG_HIP_API int hyteg_hip_download( void* host_dst, const void* dev_src, size_t bytes, hyteg_hip_stream_t stream );
HYTEG_HIP_API int hyteg_hip_copy( void* dev_dst, const void* dev_src, size_t bytes, hyteg_hip_stream_t stream );
/* Calibration: a streaming copy kernel of n doubles (plain loads, nontemporal stores if `nontemporal`),
 * the practical floor a sweep over the same bytes is compared with (bench.py: roofline.copy_us).  No reference
 * counterpart (the reference's counterpart of this measurement is the STREAM table of its kerncraft machine files,
 * data/kerncraftMachineFiles/SkylakeSP_Platinum-8147_2.7GHz.yml:412-420). */
HYTEG_HIP_API int hyteg_hip_calib_copy( double* dst, const double* src, int64_t n, int nontemporal, hyteg_hip_stream_t stream );
/* `count` such copies, copy k on pair (first + k) % npairs, between two timing events (hyteg_hip_event_create_timing; NULL =
 * none) recorded on `stream` directly before the first and after the last launch. */
typedef void* hyteg_hip_event_t;
HYTEG_HIP_API int hyteg_hip_calib_copy_ring( double* const* dsts, const double* const* srcs, int npairs, int64_t n, int nontemporal, int first,
                                             int count, hyteg_hip_stream_t stream, hyteg_hip_event_t start, hyteg_hip_event_t stop );
HYTEG_HIP_API int hyteg_hip_stream_create( hyteg_hip_stream_t* stream );
HYTEG_HIP_API int hyteg_hip_stream_destroy( hyteg_hip_stream_t stream );
HYTEG_HIP_API int hyteg_hip_stream_synchronize( hyteg_hip_stream_t stream );

/* Graphs: record the launches issued on `stream` between begin and end (nothing executes while recording) and replay
 * them with one call.  No counterpart in the reference (its kernels are host loops); this is what keeps the coarse
 * levels of GeometricMultigridSolver::solveRecursively (GeometricMultigridSolver.hpp:180-319), ~100 dependent launches
 * of a few microseconds, from being bound by the host's launch rate.  The null stream cannot be recorded; a recording
 * with no launches yields a NULL graph, which launches as a no-op.  abort_capture ends a recording after an error. */
typedef void* hyteg_hip_graph_t;
HYTEG_HIP_API int hyteg_hip_graph_begin_capture( hyteg_hip_stream_t stream );
HYTEG_HIP_API int hyteg_hip_graph_end_capture( hyteg_hip_stream_t stream, hyteg_hip_graph_t* graph );
HYTEG_HIP_API int hyteg_hip_graph_abort_capture( hyteg_hip_stream_t stream );
/* *capturing = 1 while `stream` is being recorded into a graph (by this library or by anybody else), else 0: what a caller
 * asks before it forks work onto streams of its own, which a recording would otherwise pull in */
HYTEG_HIP_API int hyteg_hip_stream_is_capturing( hyteg_hip_stream_t stream, int* capturing );
HYTEG_HIP_API int hyteg_hip_graph_launch( hyteg_hip_graph_t graph, hyteg_hip_stream_t stream );
HYTEG_HIP_API int hyteg_hip_graph_destroy( hyteg_hip_graph_t graph );

/* Builds and uploads the per-level launch tables (tile descriptors) so that later launches at that
 * level allocate nothing (HIP-graph capturable).  Launches do this lazily on first use otherwise. */
HYTEG_HIP_API int hyteg_hip_prepare_level( int level );

/* ---- layout (host-side helpers; same arithmetic as the kernels) ---------------------------------
 * src/hyteg/indexing/MacroCellIndexing.hpp:40-52, src/hyteg/Levelinfo.hpp:36-115 */
HYTEG_HIP_API int64_t hyteg_hip_cell_width( int level );      /* 2^level + 1 */
HYTEG_HIP_API int64_t hyteg_hip_cell_size( int level );       /* number of doubles in a cell array */
HYTEG_HIP_API int64_t hyteg_hip_cell_inner_size( int level ); /* DoFs the interior kernels update */
HYTEG_HIP_API int64_t hyteg_hip_cell_index( int level, int x, int y, int z );

/* ---- a2: constant-stencil apply on one macro-cell ---------------------------------------------------
 * replaces hyteg::vertexdof::macrocell::generated::apply_3D_macrocell_vertexdof_to_vertexdof_replace / _add
 *   src/constant_stencil_operator/P1generatedKernels/apply_3D_macrocell_vertexdof_to_vertexdof_replace.cpp:34-101
 *   src/constant_stencil_operator/P1generatedKernels/apply_3D_macrocell_vertexdof_to_vertexdof_add.cpp
 *   (caller src/constant_stencil_operator/P1ConstantOperator.cpp:392-428)
 * dst_i (=|+=) sum_k w_k src_{i+o_k} on the cell interior; boundary entries of dst are not touched.
 * src and dst must not alias (src/hyteg/p1functionspace/P1Operator.hpp:198). */
HYTEG_HIP_API int hyteg_hip_p1_apply_cell( double*            dst,
                                           const double*      src,
                                           int                level,
                                           const double*      w /* host, 15 */,
                                           int                update,
                                           hyteg_hip_stream_t stream );
/* nsteps INDEPENDENT applies of ONE stencil on one macro-cell geometry in ONE launch: dsts[k] (=|+=) A srcs[k], k = 0 .. nsteps-1,
 * each with the bits hyteg_hip_p1_apply_cell gives for that pair (the grid carries the bricks of all steps, so a step starts while the
 * waves of the one before it drain: no kernel boundary between them).  No reference counterpart (its kernels are host loops).
 * Contract: 1 <= nsteps <= 16 (EINVAL otherwise, nothing is launched); dsts / srcs are HOST arrays of device pointers and are read
 * before the call returns; the caller guarantees that no array written by one step is read or written by another step of the same
 * call (dsts[i] == srcs[j] or dsts[i] == dsts[j] is rejected with EINVAL; overlaps of different base pointers are not detected).
 * Levels and modes of the z-march kernel (levels 2..10, Replace and Add); any other level returns HYTEG_HIP_ENOTSUP and launches
 * nothing, and the caller issues the applies one by one.  nsteps == 1 is hyteg_hip_p1_apply_cell. */
HYTEG_HIP_API int hyteg_hip_p1_apply_cell_steps( void* const*       dsts /* host, nsteps device pointers */,
                                                 const void* const* srcs /* host, nsteps device pointers */,
                                                 int                nsteps,
                                                 int                level,
                                                 const double*      w /* host, 15 */,
                                                 int                update,
                                                 hyteg_hip_stream_t stream );

/* ---- float instantiations of a2 / a4 and mixed-precision support -------------------------------------------------
 * The reference instantiates its generated apply kernels for float32 as well
 *   src/constant_stencil_operator/P1generatedKernels/apply_3D_macrocell_vertexdof_to_vertexdof_replace.cpp:96-97
 * (its generated SOR / Gauss-Seidel kernels are double only, sor_3D_macrocell_P1.cpp).  Arrays of float in the same
 * macro-cell layout; weights are given as doubles and converted; the arithmetic is float.  Levels 2..10. */
HYTEG_HIP_API int hyteg_hip_p1_apply_cell_f32( float* dst, const float* src, int level, const double* w /* host, 15 */, int update, hyteg_hip_stream_t stream );
HYTEG_HIP_API int hyteg_hip_p1_jacobi_cell_f32( float*             dst,
                                                const float*       rhs,
                                                const float*       src,
                                                const float*       invdiag /* device or NULL */,
                                                int                level,
                                                const double*      w /* host, 15 */,
                                                double             relax,
                                                hyteg_hip_stream_t stream );
/* flat conversions and y (double) += alpha * x (float): VertexDoFFunction::copyFrom between value types
 * (src/hyteg/p1functionspace/VertexDoFFunction.hpp:598-650) on device arrays of n entries */
HYTEG_HIP_API int hyteg_hip_convert_f64_to_f32( float* dst, const double* src, size_t n, hyteg_hip_stream_t stream );
HYTEG_HIP_API int hyteg_hip_convert_f32_to_f64( double* dst, const float* src, size_t n, hyteg_hip_stream_t stream );
HYTEG_HIP_API int hyteg_hip_axpy_f32_into_f64( double* y, const float* x, double alpha, size_t n, hyteg_hip_stream_t stream );

/* The two fused steps of a mixed-precision Jacobi smoother that keeps iterate and right-hand side in double and sweeps the error
 * equation in float (no reference counterpart as a kernel; the reference's pieces are the float instantiation of its apply kernel
 * and VertexDoFFunction::copyFrom between precisions, see above).  n Jacobi sweeps on A x = b equal
 *    r = b - A x;  e_1 = relax r / c;  e_{k+1} = e_k + relax ( r - A e_k ) / c  (k = 1 .. n-1);  x += e_n      (c = centre weight)
 * on the inner points of a macro-cell whose boundary values are fixed (e = 0 there):
 *   hyteg_hip_p1_residual_jacobi_start_f32: r (double arithmetic) rounded to float into r_f32, and e_1 into e_f32 -- one launch;
 *   hyteg_hip_p1_jacobi_cell_f32 (above): the sweeps in between;
 *   hyteg_hip_p1_jacobi_accumulate_f32: the last sweep, added to x (double) instead of being stored -- one launch.
 * n launches for n sweeps, 60 instead of 72 bytes per DoF for n = 3.  Levels 2..10; only inner points are read-modified. */
HYTEG_HIP_API int hyteg_hip_p1_residual_jacobi_start_f32( float* r_f32, float* e_f32, const double* rhs, const double* src, int level, const double* w,
                                                          double relax, hyteg_hip_stream_t stream );
HYTEG_HIP_API int hyteg_hip_p1_jacobi_accumulate_f32( double* x, const float* rhs_f32, const float* e_f32, int level, const double* w, double relax,
                                                      hyteg_hip_stream_t stream );

/* Name of the kernel instantiation hyteg_hip_p1_apply_cell( ..., level, ..., update, ... ) launches on the current device,
 * with its template arguments, e.g. "p1_apply_zmarch_preload_kernel<MODE=0,NY=4,LZ=8,EX_AUX=0,DEC=0,PFD=2>" — what profiler
 * output and recorded counter files are matched against (no reference counterpart: measurement support).  EX_AUX (2 for Add,
 * 0 otherwise) and DEC (always 0) are no template arguments of the kernel any more: they are constants kept for continuity of
 * the recorded names. */
HYTEG_HIP_API int hyteg_hip_p1_apply_kernel_name( int level, int update, char* buf, size_t buflen );
/* Tuning knob (measurement support, like hyteg_hip_set_sor_algorithm): brick shape of the z-march apply / Jacobi / residual
 * kernels for all later launches of this process -- ny rows x lz slices per wave, loads pfd slices ahead of the arithmetic.
 * Only shapes compiled into the library are accepted (EINVAL otherwise); ( 0, 0, 0 ) restores the per-level defaults.
 * Results do not depend on the shape (same terms in the same order at every point). */
HYTEG_HIP_API int hyteg_hip_set_apply_shape( int ny, int lz, int pfd );
/* Tuning knob of hyteg_hip_p1_apply_cell_steps alone: x-stride of its bricks for all later launches of this process -- 62 (every
 * wave stores lanes 1..62 of its rows) or 56 (every row segment begins on a 64-byte line of the destination); 0 restores the
 * default of the mode and level; any other value is EINVAL.  Results do not depend on it. */
HYTEG_HIP_API int hyteg_hip_set_apply_steps_xs( int xs );
/* Test support, host only (no device is touched): count[i] = how many waves of the z-march store entry i of a level's cell array
 * (count: host, cell size of the level) with bricks of ny rows x lz slices and x-stride xs, for a destination whose first byte is
 * dst_phase (0..7) entries past a 64-byte line; *nbricks = bricks of the table.  A correct table gives 1 on the entries the apply
 * writes and 0 elsewhere.  Levels 2..8; a store window that leaves the wave or the array is EINVAL. */
HYTEG_HIP_API int hyteg_hip_p1_apply_brick_coverage( int level, int ny, int lz, int xs, int dst_phase, unsigned char* count /* host */, int* nbricks );

/* ---- a4: weighted Jacobi sweep, fused ------------------------------------------------------------------
 * replaces the 1 apply + 3 vector passes of P1Operator::smooth_jac
 *   src/hyteg/p1functionspace/P1Operator.hpp:429-447
 * dst = src + relax * invDiag .* ( rhs - A src )  on the cell interior.
 * invdiag: cell array of inverse diagonal values (getInverseDiagonalValues()), or NULL to use the
 * constant 1/w[7] (what computeInverseDiagonalOperatorValues() stores on a constant-stencil cell,
 * P1Operator.hpp:636-906).  dst must not alias src. */
HYTEG_HIP_API int hyteg_hip_p1_jacobi_cell( double*            dst,
                                            const double*      rhs,
                                            const double*      src,
                                            const double*      invdiag /* device or NULL */,
                                            int                level,
                                            const double*      w /* host, 15 */,
                                            double             relax,
                                            hyteg_hip_stream_t stream );

/* ---- a4 / a13: the steps of a Chebyshev smoother, fused ------------------------------------------------------
 * replaces, per step of ChebyshevSmoother::solve (src/hyteg/solvers/ChebyshevSmoother.hpp:165-212), the apply
 * (P1Operator.hpp:192-320), the assign of the residual (first step only), the multElementwise with the inverse diagonal
 * (ApplyFunctionMultiplicationWrapper::apply, src/hyteg/solvers/ApplyInverseDiagonalWrapper.hpp) and
 * the assign x = x + c t (VertexDoFFunction.cpp:1088-1128) on the cell interior: one launch instead of four,
 * 40 instead of 72 bytes per DoF (32 with the scalar inverse diagonal).
 *   start:  t_out = invDiag .* ( rhs - A x ).  x is the stencil source of this launch and is NOT updated here (other waves
 *           still read its old values): the update x += c_0 t_out is deferred to the next step (or to hyteg_hip_p1_add_cell
 *           for a smoother of order 1).
 *   step:   t_out = invDiag .* ( A t_in ), and at the same point x = ( x + c_prev t_in ) + c_cur t_out, the first term only
 *           if has_prev != 0.  x is read and written by the same lane at the same address only (in place).
 * invdiag: cell array of inverse diagonal values or NULL for the constant 1/w[7], as in hyteg_hip_p1_jacobi_cell.
 * t_out must alias neither x, rhs, t_in nor invdiag, and x not t_in (EINVAL).  Every point sums the 15 terms in the order
 * of hyteg_hip_p1_apply_cell, multiplies by the inverse diagonal and updates x: the composition's values up to the
 * contraction of x + c t into one FMA.  Levels 2..11 (level 11 is composed from the entry points above inside the library). */
HYTEG_HIP_API int hyteg_hip_p1_chebyshev_start_cell( double*            t_out,
                                                     const double*      rhs,
                                                     const double*      x,
                                                     const double*      invdiag /* device or NULL */,
                                                     int                level,
                                                     const double*      w /* host, 15 */,
                                                     hyteg_hip_stream_t stream );
HYTEG_HIP_API int hyteg_hip_p1_chebyshev_step_cell( double*            t_out,
                                                    double*            x,
                                                    const double*      t_in,
                                                    const double*      invdiag /* device or NULL */,
                                                    int                level,
                                                    const double*      w /* host, 15 */,
                                                    double             c_prev,
                                                    double             c_cur,
                                                    int                has_prev,
                                                    hyteg_hip_stream_t stream );

/* Selects how hyteg_hip_p1_sor_cell / hyteg_hip_p1_sor_cells execute the sweep.  Every form visits the points in an
 * order that respects the reference's lexicographic (z,y,x) dependencies (sor_3D_macrocell_P1.cpp:48-88), so the results
 * agree up to the rounding of the 15-term sum.  Process-wide; meant for tests and benchmarks.
 *   AUTO      levels >= 5: BLOCKS; below: PLANES (batches at levels <= 5: one workgroup per cell)
 *   PLANES    one launch per hyperplane x + 2y + 3z
 *   BLOCKS    16^3 blocks in skewed coordinates, one launch per block wavefront
 *   DATAFLOW  one launch; 8 x 8-row columns, one wave each, hand results over through progress words (levels >= 3);
 *             measured slower than BLOCKS on MI355X, kept as an opt-in */
enum hyteg_hip_sor_algorithm
{
   HYTEG_HIP_SOR_AUTO     = 0,
   HYTEG_HIP_SOR_PLANES   = 1,
   HYTEG_HIP_SOR_BLOCKS   = 2,
   HYTEG_HIP_SOR_DATAFLOW = 3
};
HYTEG_HIP_API int hyteg_hip_set_sor_algorithm( int algorithm );

/* ---- a3: SOR / Gauss-Seidel sweep, in place, in the reference's lexicographic order -----------------
 * replaces sor_3D_macrocell_P1, sor_3D_macrocell_P1_backwards, gaussseidel_3D_macrocell_P1 (relax = 1)
 *   src/constant_stencil_operator/P1generatedKernels/sor_3D_macrocell_P1.cpp:32-90
 *   src/constant_stencil_operator/P1generatedKernels/sor_3D_macrocell_P1_backwards.cpp:52-57
 *   src/constant_stencil_operator/P1generatedKernels/gaussseidel_3D_macrocell_P1.cpp:32-88
 *   (caller P1ConstantOperator.cpp:639-677)
 * The sweep is executed as hyperplanes x + 2y + 3z = const, which reproduces the sequential
 * (z, y, x) update order of the reference exactly (every already-updated neighbour lies on an
 * earlier plane, every not-yet-updated one on a later plane). */
HYTEG_HIP_API int hyteg_hip_p1_sor_cell( double*            u,
                                         const double*      rhs,
                                         int                level,
                                         const double*      w /* host, 15 */,
                                         double             relax,
                                         int                backwards,
                                         hyteg_hip_stream_t stream );
/* nsweeps consecutive sweeps of the same direction: what a smoother's pre- / post-smoothing loop does to a macro-cell
 * whose boundary values do not change between the sweeps (GeometricMultigridSolver.hpp:209-215 calling
 * P1ConstantOperator::smooth_sor).  Same result, bit for bit, as nsweeps calls of hyteg_hip_p1_sor_cell; from level 5 on
 * the sweeps run as one pipeline of block wavefronts (sweep s + 1 four wavefronts behind sweep s), 46 + 4 ( nsweeps - 1 )
 * launches instead of 46 nsweeps at level 8. */
HYTEG_HIP_API int hyteg_hip_p1_sor_cell_sweeps( double*            u,
                                                const double*      rhs,
                                                int                level,
                                                const double*      w /* host, 15 */,
                                                double             relax,
                                                int                backwards,
                                                int                nsweeps,
                                                hyteg_hip_stream_t stream );

/* dst = rhs - A src on the cell interior in one launch: what a multigrid cycle computes with apply + assign( { 1, -1 } )
 * (GeometricMultigridSolver.hpp:240-246: A.apply( x, tmp ); tmp.assign( { 1.0, -1.0 }, { b, tmp } )); the same bits as the two
 * calls.  dst may be rhs, not src.  Levels 2..10. */
HYTEG_HIP_API int hyteg_hip_p1_residual_cell( double*            dst,
                                              const double*      rhs,
                                              const double*      src,
                                              int                level,
                                              const double*      w /* host, 15 */,
                                              hyteg_hip_stream_t stream );

/* ---- a6: vector kernels on the cell interior ---------------------------------------------------------
 * assign:  dst = sum_k c_k src_k      replaces assign_3D_macrocell_vertexdof_{1,2,3}_rhs_function(s)
 *   src/hyteg/p1functionspace/generatedKernels/assign_3D_macrocell_vertexdof_*.cpp
 *   (dispatch src/hyteg/p1functionspace/VertexDoFFunction.cpp:1088-1128; generic
 *    src/hyteg/p1functionspace/VertexDoFMacroCell.hpp:376-402)
 * add:     dst += sum_k c_k src_k     VertexDoFMacroCell.hpp:456-481, add_3D_macrocell_vertexdof_1_rhsfunction.cpp
 * mult:    dst = prod_k src_k         VertexDoFMacroCell.hpp:483-508 (multElementwise)
 * srcs: HOST array of nsrc device pointers (1 <= nsrc <= HYTEG_HIP_MAX_SRCS); sources may alias dst. */
HYTEG_HIP_API int hyteg_hip_p1_assign_cell( double*              dst,
                                            int                  nsrc,
                                            const double* const* srcs,
                                            const double*        scalars /* host, nsrc */,
                                            int                  level,
                                            hyteg_hip_stream_t   stream );
HYTEG_HIP_API int hyteg_hip_p1_add_cell( double*              dst,
                                         int                  nsrc,
                                         const double* const* srcs,
                                         const double*        scalars /* host, nsrc */,
                                         int                  level,
                                         hyteg_hip_stream_t   stream );
HYTEG_HIP_API int
    hyteg_hip_p1_mult_cell( double* dst, int nsrc, const double* const* srcs, int level, hyteg_hip_stream_t stream );

/* dot: sum over the cell interior of a_i * b_i   replaces vertexdof::macrocell::dot
 *   src/hyteg/p1functionspace/VertexDoFMacroCell.hpp:511-529
 * Two deterministic passes (per-workgroup partial sums, then one workgroup adds them in fixed
 * order); the result is written to *result_dev (device memory, stream-ordered).  workspace_dev must
 * hold hyteg_hip_dot_workspace_bytes() bytes and must not be shared by dots in flight on different
 * streams.  The reference's plain sequential sum differs by reassociation only. */
HYTEG_HIP_API size_t hyteg_hip_dot_workspace_bytes( void );
HYTEG_HIP_API int    hyteg_hip_p1_dot_cell( const double*      a,
                                            const double*      b,
                                            int                level,
                                            double*            result_dev,
                                            void*              workspace_dev,
                                            hyteg_hip_stream_t stream );

/* ---- a7 / a8: grid transfer on one macro-cell ----------------------------------------------------------
 * restrict: replaces restrict_3D_macrocell_P1_pull_additive<double>
 *   src/hyteg/gridtransferoperators/generatedKernels/restrict_3D_macrocell_P1_pull_additive.cpp:33-1690
 *   (caller src/hyteg/gridtransferoperators/P1toP1LinearRestriction.cpp:169-243)
 *   writes EVERY coarse point (boundary included) with this cell's partial sum.
 * prolongate: replaces the zeroing at P1toP1LinearProlongation.cpp:214-238 plus
 *   prolongate_3D_macrocell_P1_push_additive<double>
 *   src/hyteg/gridtransferoperators/generatedKernels/prolongate_3D_macrocell_P1_push_additive.cpp
 *   The reference scatters from coarse points; here every fine point gathers its (at most two)
 *   coarse parents, adding them in the order the scatter would have.  update = REPLACE overwrites
 *   the whole fine array; update = ADD overwrites the boundary shell and adds to the interior. */
HYTEG_HIP_API int hyteg_hip_p1_restrict_cell( double*            coarse,
                                              const double*      fine,
                                              int                coarse_level,
                                              const double*      nnc /* host, 14 */,
                                              hyteg_hip_stream_t stream );
HYTEG_HIP_API int hyteg_hip_p1_prolongate_cell( const double*      coarse,
                                                double*            fine,
                                                int                coarse_level,
                                                const double*      nnc /* host, 14 */,
                                                int                update,
                                                hyteg_hip_stream_t stream );

/* ---- cell-centric multi-cell support -------------------------------------------------------------------
 * On meshes with several macro-cells this library keeps the DoFs of macro-faces/edges/vertices in the boundary
 * entries of every adjacent cell array (HyTeG's cell arrays hold the same copies after communicate<Face,Cell>,
 * src/hyteg/p1functionspace/VertexDoFPackInfo.hpp:410-478).  Points are addressed by a 15-bit mask:
 * bit k (k = 0..13) selects the points on the macro-primitive in slot k of { edge0..5, face0..3, vertex0..3 }
 * (the cell-local numbering of src/hyteg/indexing/MacroCellIndexing.cpp:36-91), bit 14 the cell interior.
 * A host layer derives the mask from the DoFType flag and the primitives' boundary conditions, which is the
 * test `testFlag( bc.getBoundaryType( prim.getMeshBoundaryFlag() ), flag )` of P1Operator.hpp:213-303. */
#define HYTEG_HIP_SLOT_INNER 14
#define HYTEG_HIP_MASK_INNER ( 1u << 14 )
#define HYTEG_HIP_MASK_SHELL 0x3FFFu
#define HYTEG_HIP_MASK_ALL 0x7FFFu

/* a9: apply on the points of the cell boundary with this cell's PARTIAL stencils
 * (what P1Elements3D::calculateStencilInMacroCell gives for a micro-vertex on that face/edge/vertex,
 *  src/hyteg/p1functionspace/P1Elements.hpp:215-380; the reference stores them per neighbour cell in
 *  faceStencil3D / edgeStencil3D, src/constant_stencil_operator/P1ConstantOperator.cpp:239-357).
 * w_slots: host, 14 x 15 weights (slot-major, stencil order as above; weights of neighbours outside the cell
 * are ignored).  dst_i (=|+=) sum over the neighbours inside the cell.  Summing the results of all cells that
 * share a point gives the reference's value of apply() on that macro-face/edge/vertex DoF. */
HYTEG_HIP_API int hyteg_hip_p1_apply_cell_boundary( double*            dst,
                                                    const double*      src,
                                                    int                level,
                                                    const double*      w_slots /* host, 14*15 */,
                                                    unsigned           mask,
                                                    int                update,
                                                    hyteg_hip_stream_t stream );

/* a6 with a point mask: op 0 = assign, 1 = add, 2 = multElementwise (VertexDoFFunction.cpp:1130-1221,
 * 1408-1484, 1487-1563 loop over vertices, edges, faces and cells with the same flag test). */
HYTEG_HIP_API int hyteg_hip_p1_vector_cell_masked( int                  op,
                                                   double*              dst,
                                                   int                  nsrc,
                                                   const double* const* srcs,
                                                   const double*        scalars /* host, nsrc; ignored for op 2 */,
                                                   int                  level,
                                                   unsigned             mask,
                                                   hyteg_hip_stream_t   stream );
/* dst = value on the masked points (VertexDoFFunction::interpolate( constant, level, flag )) */
HYTEG_HIP_API int
    hyteg_hip_p1_set_cell_masked( double* dst, double value, int level, unsigned mask, hyteg_hip_stream_t stream );
/* dot over the masked points (dotLocal sums vertices + edges + faces + cells, VertexDoFFunction.cpp:1720-1793;
 * the host passes, per cell, the mask of the primitives that cell "owns" so that every DoF counts once). */
HYTEG_HIP_API int hyteg_hip_p1_dot_cell_masked( const double*      a,
                                                const double*      b,
                                                int                level,
                                                unsigned           mask,
                                                double*            result_dev,
                                                void*              workspace_dev,
                                                hyteg_hip_stream_t stream );
/* grid transfer writing only the masked coarse / fine points (interior bit must be set) */
HYTEG_HIP_API int hyteg_hip_p1_restrict_cell_masked( double*            coarse,
                                                     const double*      fine,
                                                     int                coarse_level,
                                                     const double*      nnc /* host, 14 */,
                                                     unsigned           mask,
                                                     hyteg_hip_stream_t stream );
HYTEG_HIP_API int hyteg_hip_p1_prolongate_cell_masked( const double*      coarse,
                                                       double*            fine,
                                                       int                coarse_level,
                                                       const double*      nnc /* host, 14 */,
                                                       unsigned           mask,
                                                       hyteg_hip_stream_t stream );
/* the same with an update type: ADD adds the interpolant to the selected interior points (bit 14) and, like
 * hyteg_hip_p1_prolongate_cell, overwrites the selected shell points -- with an interior-only mask it is
 * P1toP1LinearProlongation::prolongateAndAdd on a macro-cell whose shell is not selected, in one launch */
HYTEG_HIP_API int hyteg_hip_p1_prolongate_cell_masked_update( const double*      coarse,
                                                              double*            fine,
                                                              int                coarse_level,
                                                              const double*      nnc /* host, 14 */,
                                                              unsigned           mask,
                                                              int                update,
                                                              hyteg_hip_stream_t stream );

/* a3 on the macro-cell boundary: SOR / Gauss-Seidel on the macro-vertices, macro-edges and macro-faces around one cell
 * (vertexdof::macrovertex::smooth_sor, VertexDoFMacroVertex.hpp:231-251; P1Operator::smooth_sor_edge,
 * P1Operator.hpp:1352-1421; P1Operator::smooth_sor_face3D / the generated sor_3D_macroface_P1, :1424-1503), in the order
 * of P1Operator::smooth_sor (:348-418): vertices, edges, faces -- faces, edges, vertices if `backwards`.
 * The reference sweeps each macro-primitive in its own memory with ghost layers; here the sweep runs in the cell's
 * array on the points selected by `mask` (bits 0..13), with
 *   rest       : for every selected point the stencil sum over all neighbours that are NOT on the same macro-primitive
 *                (nor on its lower-dimensional boundary), already summed over all neighbour cells -- the ghost-layer
 *                part of the reference's sum.  Overwritten on macro-face points (scratch).
 *   edge_verts : [6][2] cell-local vertex numbers (a, b): edge e is swept from a to b (the macro-edge's orientation)
 *   edge_w     : [6][3] total weights: centre, neighbour towards a, neighbour towards b
 *   face_verts : [4][3] cell-local numbers of the macro-face's vertices 0, 1, 2 (rows y along 0->2, x along 0->1)
 *   face_w     : [4][7] total weights: centre, then (-1,0) (1,0) (0,-1) (0,1) (1,-1) (-1,1) in face coordinates
 *   vertex_w   : [4]    total centre weights
 * (host arrays).  Every cell around a shared primitive runs the same sweep on its own copy, so the copies stay
 * bit-identical without an exchange.  Levels 0..11. */
HYTEG_HIP_API int hyteg_hip_p1_sor_shell_cell( double*            dst,
                                               const double*      rhs,
                                               double*            rest,
                                               int                level,
                                               const int*         edge_verts,
                                               const double*      edge_w,
                                               const int*         face_verts,
                                               const double*      face_w,
                                               const double*      vertex_w,
                                               double             relax,
                                               unsigned           mask,
                                               int                backwards,
                                               hyteg_hip_stream_t stream );

/* ---- batched forms: ONE launch for up to HYTEG_HIP_MAX_BATCH macro-cells of the same level, inner and
 * boundary points together.  They replace the per-primitive loops of the reference (`for ( cell : storage->getCells() )`,
 * P1Operator.hpp:286-309; VertexDoFFunction.cpp:1130-1221, 1710-1793; P1toP1LinearRestriction.cpp:193-243) on the levels
 * where a cell is too small to fill the GPU.  `dst`, `src`, ... are HOST arrays of `ncells` device pointers, `masks` a host
 * array of `ncells` point masks (bits 0..13 macro-primitive slots, bit 14 inner points); tables ending in `_dev` are device
 * memory.  Levels 0..11. */
#define HYTEG_HIP_MAX_BATCH 80
/* op 0 assign, 1 add, 2 multElementwise, 3 set to scalars[0]; srcs = [nsrc][ncells] */
HYTEG_HIP_API int hyteg_hip_p1_vector_cells( int                  op,
                                             int                  ncells,
                                             double* const*       dst,
                                             int                  nsrc,
                                             const double* const* srcs,
                                             const double*        scalars,
                                             int                  level,
                                             const unsigned*      masks,
                                             hyteg_hip_stream_t   stream );
/* assign / add whose coefficients are read from device memory when the kernel runs (scalar_ptrs: host array of nsrc
 * device pointers): lets an iteration whose scalars are themselves results of device reductions proceed without a
 * host round trip per scalar (the conjugate gradient recurrences below) */
HYTEG_HIP_API int hyteg_hip_p1_vector_cells_dev( int                  op,
                                                 int                  ncells,
                                                 double* const*       dst,
                                                 int                  nsrc,
                                                 const double* const* srcs,
                                                 const double* const* scalar_ptrs,
                                                 int                  level,
                                                 const unsigned*      masks,
                                                 hyteg_hip_stream_t   stream );
/* Scalar recurrences of CGSolver::solve (src/hyteg/solvers/CGSolver.hpp:91-140; identity preconditioner) on the device.
 * s_dev: HYTEG_HIP_CG_SLOTS doubles.  The caller writes the dot products into RR / PAP (hyteg_hip_p1_dot_cells) and calls
 *   phase 0  after RR = <r,r> of the initial residual: prsold = RR, res_start = sqrt(RR), done = res_start < abs_tol
 *   phase 1  after PAP = <p,Ap>:  alpha = prsold / PAP, NEG_ALPHA = -alpha        (both 0 once done)
 *   phase 2  after RR = <r,r>:    iterations += 1; done if sqrt(RR)/res_start < rel_tol or sqrt(RR) < abs_tol,
 *                                 else beta = RR / prsold, prsold = RR            (nothing once done)
 * With alpha = 0 the updates x += alpha p, r -= alpha Ap leave x and r as they are, so iterations enqueued beyond
 * convergence change nothing and the host only needs to look at DONE every few iterations. */
enum hyteg_hip_cg_slot
{
   HYTEG_HIP_CG_PRSOLD     = 0,
   HYTEG_HIP_CG_PAP        = 1,
   HYTEG_HIP_CG_RR         = 2,
   HYTEG_HIP_CG_ALPHA      = 3,
   HYTEG_HIP_CG_NEG_ALPHA  = 4,
   HYTEG_HIP_CG_BETA       = 5,
   HYTEG_HIP_CG_RES_START  = 6,
   HYTEG_HIP_CG_DONE       = 7,
   HYTEG_HIP_CG_ITERATIONS = 8,
   HYTEG_HIP_CG_ONE        = 9,
   HYTEG_HIP_CG_SLOTS      = 16
};
HYTEG_HIP_API int hyteg_hip_cg_scalars( double* s_dev, int phase, double rel_tol, double abs_tol, hyteg_hip_stream_t stream );
/* The whole conjugate gradient solve of CGSolver::solve (CGSolver.hpp:91-140, identity preconditioner) in ONE launch of one
 * workgroup, for problems whose cell arrays together have at most hyteg_hip_p1_cg_small_max_entries() entries (the
 * coarsest level of a multigrid hierarchy).  x: initial guess in, solution out (entries the masks do not select are read
 * as boundary values); operator and masks as in hyteg_hip_p1_apply_cells; owned_masks select the points a dot product
 * counts (each shared point once).  The copies of shared points are summed inside the kernel: group tables of up to two
 * exchange classes (group_ptr[k]: ngroups[k] + 1 offsets into entry_cell[k] / entry_off[k], all device arrays; entries
 * name a cell of this batch and an array offset).  info_dev (may be NULL): [0] iterations, [1] final residual norm. */
HYTEG_HIP_API int hyteg_hip_p1_cg_small_max_entries( void );
HYTEG_HIP_API int hyteg_hip_p1_cg_small_cells( int                  ncells,
                                               double* const*       x,
                                               const double* const* b,
                                               int                  level,
                                               const double*        stencils_dev,
                                               const unsigned*      masks,
                                               const unsigned*      owned_masks,
                                               const int* const*    group_ptr_dev,
                                               const int* const*    entry_cell_dev,
                                               const int* const*    entry_off_dev,
                                               const int*           ngroups,
                                               int                  max_iter,
                                               double               rel_tol,
                                               double               abs_tol,
                                               double*              info_dev,
                                               hyteg_hip_stream_t   stream );
/* hyteg_hip_p1_dot_cells into s_dev[slot] (slot = HYTEG_HIP_CG_PAP or HYTEG_HIP_CG_RR) followed by hyteg_hip_cg_scalars( phase )
 * in the same launch */
HYTEG_HIP_API int hyteg_hip_p1_dot_cells_cg( int                  ncells,
                                             const double* const* a,
                                             const double* const* b,
                                             int                  level,
                                             const unsigned*      masks,
                                             double*              s_dev,
                                             int                  slot,
                                             int                  phase,
                                             double               rel_tol,
                                             double               abs_tol,
                                             void*                workspace_dev,
                                             hyteg_hip_stream_t   stream );
/* *result_dev = sum over all cells and masked points of a.b; up to 64 workgroups: one launch (the workgroup that finishes
 * last reduces the partial sums), more: a second launch does; fixed order either way: the result does not depend on timing;
 * workspace: hyteg_hip_dot_workspace_bytes() */
HYTEG_HIP_API int hyteg_hip_p1_dot_cells( int                  ncells,
                                          const double* const* a,
                                          const double* const* b,
                                          int                  level,
                                          const unsigned*      masks,
                                          double*              result_dev,
                                          void*                workspace_dev,
                                          hyteg_hip_stream_t   stream );
/* The vector body of a conjugate gradient iteration in ONE pass over the arrays (48 bytes per DoF instead of the 56 of the composed
 * calls): replaces  x.add( { alpha }, { p } );  r.add( { -alpha }, { ap } );  rsnew = r.dotGlobal( r )  of CGSolver::solve
 * (src/hyteg/solvers/CGSolver.hpp:152-154), i.e. VertexDoFFunction::add (VertexDoFFunction.cpp:1408-1484) twice and dotLocal
 * (:1710-1793).  On the points update_masks[c] selects in cell c:  x += alpha p,  r -= alpha ap  (each one fused multiply-add); every
 * other entry of x and r keeps its bits, p and ap are only read.  Then *result_dev = sum over all cells and the points dot_masks[c]
 * selects of r * r, with the values of r after the update.  Two masks because a caller updates every copy of a DoF that cells share
 * and counts it once.  Masks: the 15-bit point masks of hyteg_hip_p1_vector_cells; a cell whose two masks are 0 is not touched.
 * Up to 128 workgroups (tiles of 1024 entries, cells together): one launch, the workgroup that finishes last reduces the partial
 * sums; more: a second launch does; fixed order either way: the result does not depend on timing.  Stream-ordered, no allocation
 * beyond the cached tile table, no synchronisation.  Levels 0..11; x, r, p, ap and the masks: HOST arrays of ncells entries;
 * workspace_dev: hyteg_hip_dot_workspace_bytes().  EINVAL before any GPU work for a bad level or ncells, a null pointer, and x[c] or
 * r[c] equal to another array of the same cell. */
HYTEG_HIP_API int hyteg_hip_p1_cg_update_cells( int                  ncells,
                                                double* const*       x,
                                                double* const*       r,
                                                const double* const* p,
                                                const double* const* ap,
                                                double               alpha,
                                                int                  level,
                                                const unsigned*      update_masks,
                                                const unsigned*      dot_masks,
                                                double*              result_dev,
                                                void*                workspace_dev,
                                                hyteg_hip_stream_t   stream );
/* The statistics of a function on every macro-cell of a rank in ONE pass over its arrays (8 bytes read per DoF, nothing written):
 * results_dev[c * HYTEG_HIP_REDUCE_COUNT + q] = statistic q of the points of cell c that masks[c] selects (the 15-bit point mask of
 * hyteg_hip_p1_dot_cells).  Replaces the per-primitive loops of VertexDoFFunction::sumLocal (VertexDoFFunction.cpp:1805-1851, with and
 * without `absolute`), getMaxDoFValue (:1909-1957), getMaxDoFMagnitude (:1959-2007) and getMinDoFValue (:2009-2057); an empty
 * selection gives their starting values 0, 0, +DBL_MAX, -DBL_MAX, 0 (:1809, :1912, :1962, :2012).
 * The numbers of cell c depend on that cell's array, the level and its mask alone -- not on ncells, the cell's position in the batch
 * or timing: the workgroups of a cell and the tiles each reads follow from the level, and the partial results of a cell are folded in
 * a fixed order (up to 32 tiles of 256 entries: one workgroup per cell, one launch; above: up to 1024 per cell and a second launch of
 * one workgroup per cell).  Stream-ordered, no allocation beyond the cached tile table, no synchronisation.  NaN entries are outside
 * the contract.  Levels 0..11; a and masks: HOST arrays of ncells entries; workspace_dev: hyteg_hip_reduce_workspace_bytes() bytes,
 * not to be shared by reductions in flight on different streams. */
#define HYTEG_HIP_REDUCE_SUM 0     /* sum of x   */
#define HYTEG_HIP_REDUCE_SUM_ABS 1 /* sum of |x| */
#define HYTEG_HIP_REDUCE_MIN 2
#define HYTEG_HIP_REDUCE_MAX 3
#define HYTEG_HIP_REDUCE_MAX_ABS 4
#define HYTEG_HIP_REDUCE_COUNT 5
HYTEG_HIP_API size_t hyteg_hip_reduce_workspace_bytes( void );
HYTEG_HIP_API int    hyteg_hip_p1_reduce_cells( int                  ncells,
                                                const double* const* a,
                                                int                  level,
                                                const unsigned*      masks,
                                                double*              results_dev,
                                                void*                workspace_dev,
                                                hyteg_hip_stream_t   stream );
/* stencils_dev: [ncells][15][15]; rows 0..13 = the cell's share of the stencil at a point of macro-primitive slot s
 * (w_slots of hyteg_hip_p1_apply_cell_boundary), row 14 = the inner stencil (w of hyteg_hip_p1_apply_cell) */
HYTEG_HIP_API int hyteg_hip_p1_apply_cells( int                  ncells,
                                            double* const*       dst,
                                            const double* const* src,
                                            int                  level,
                                            const double*        stencils_dev,
                                            const unsigned*      masks,
                                            int                  update,
                                            hyteg_hip_stream_t   stream );
/* smooth_jac in two phases around the additive exchange of dst: phase 0 writes the complete update on inner points and the
 * cell's share of A.src on boundary points; phase 1 turns the summed shares into dst = src + relax*invdiag*( rhs - dst ) */
HYTEG_HIP_API int hyteg_hip_p1_jacobi_cells( int                  ncells,
                                             double* const*       dst,
                                             const double* const* rhs,
                                             const double* const* src,
                                             const double* const* invdiag,
                                             int                  level,
                                             const double*        stencils_dev,
                                             double               relax,
                                             const unsigned*      masks,
                                             int                  phase,
                                             hyteg_hip_stream_t   stream );
/* nnc_inv_dev: [ncells][14] = 1 / numNeighborCells in the slot order of hyteg_hip_p1_restrict_cell */
HYTEG_HIP_API int hyteg_hip_p1_restrict_cells( int                  ncells,
                                               double* const*       coarse,
                                               const double* const* fine,
                                               int                  coarse_level,
                                               const double*        nnc_inv_dev,
                                               const unsigned*      masks,
                                               hyteg_hip_stream_t   stream );
HYTEG_HIP_API int hyteg_hip_p1_prolongate_cells( int                  ncells,
                                                 const double* const* coarse,
                                                 double* const*       fine,
                                                 int                  coarse_level,
                                                 const double*        nnc_inv_dev,
                                                 const unsigned*      masks,
                                                 int                  update,
                                                 hyteg_hip_stream_t   stream );

/* in-place SOR / GS sweep over the inner points of every cell whose mask has bit 14 (hyteg_hip_p1_sor_cell for a batch);
 * levels <= 5: one workgroup per cell with the array in LDS, above: the blocked sweep with the cell as second grid dimension.
 * stencils_dev as for hyteg_hip_p1_apply_cells (row 14 is used). */
HYTEG_HIP_API int hyteg_hip_p1_sor_cells( int                  ncells,
                                          double* const*       u,
                                          const double* const* rhs,
                                          int                  level,
                                          const double*        stencils_dev,
                                          double               relax,
                                          int                  backwards,
                                          const unsigned*      masks,
                                          hyteg_hip_stream_t   stream );
/* per-cell tables of hyteg_hip_p1_sor_shell_cell as one record (device array of `ncells` records for the batched form) */
typedef struct hyteg_hip_sor_shell_tables
{
   int    edge_verts[6][2];
   int    face_verts[4][3];
   double edge_w[6][3];
   double face_w[4][7];
   double vertex_w[4];
} hyteg_hip_sor_shell_tables;
HYTEG_HIP_API int hyteg_hip_p1_sor_shell_cells( int                               ncells,
                                                double* const*                    dst,
                                                const double* const*              rhs,
                                                double* const*                    rest,
                                                int                               level,
                                                const hyteg_hip_sor_shell_tables* tables_dev,
                                                double                            relax,
                                                const unsigned*                   masks,
                                                int                               backwards,
                                                hyteg_hip_stream_t                stream );

/* ---- f1: P2 (vertex + edge DoFs) elementwise operator on one macro-cell ----
 * P2ElementwiseOperator::gemv, src/hyteg/elementwiseoperators/P2ElementwiseOperator.cpp:110-223 (cell loop) with
 * localMatrixVectorMultiply3D (:66-107).  Arrays: the vertex-DoF array of the P1 kernels and the edge-DoF array of
 * src/hyteg/edgedofspace/EdgeDoFIndexing.hpp:920-985: blocks X, Y, Z, XY, XZ, YZ of tet(2^level) entries and XYZ of
 * tet(2^level - 1).  The operator of an affine macro-cell is given by the six 10 x 10 element matrices of the micro-cell
 * types WHITE_UP, BLUE_UP, GREEN_UP, WHITE_DOWN, BLUE_DOWN, GREEN_DOWN (celldof::allCellTypes) in FEniCS ordering
 * (P2Form::integrateAll, kernel INPUT): hyteg_hip_p2_build_operator_table turns elmat[6][10][10] (host) into the table the
 * kernel reads -- the matrices themselves, used micro-cell by micro-cell for DoFs on the macro-cell boundary, followed by
 * the constant stencils they imply for inner DoFs (hyteg_hip_p2_operator_table_size() doubles); the caller uploads it
 * once per (cell, level).  Every DoF whose point class is in `mask` (vertex DoFs as for the P1 kernels; an
 * edge DoF belongs to the macro-primitive that contains both its end points) receives alpha * (A src) (REPLACE) or has
 * it added (ADD).  Boundary DoFs: the sum over micro-cells is taken in the reference's loop order; inner DoFs: in stencil order.
 * Levels 0..9. */
#define HYTEG_HIP_P2_MAX_LEVEL 9
HYTEG_HIP_API size_t hyteg_hip_p2_edge_array_size( int level );
HYTEG_HIP_API size_t hyteg_hip_p2_operator_table_size( void );
HYTEG_HIP_API int    hyteg_hip_p2_build_operator_table( const double* elmat_host /* 600 */, double* table_host );
/* EdgeDoFFunction assign / add / multElementwise / interpolate( constant ) and dotLocal on the edge-DoF array of one
 * macro-cell (src/hyteg/edgedofspace/EdgeDoFFunction.cpp), restricted to the DoFs whose point class is in `mask`;
 * op and workspace as for hyteg_hip_p1_vector_cell_masked / hyteg_hip_p1_dot_cell_masked */
HYTEG_HIP_API int hyteg_hip_p2_edge_vector_cell_masked( int                  op,
                                                        double*              dst,
                                                        int                  nsrc,
                                                        const double* const* srcs,
                                                        const double*        scalars,
                                                        int                  level,
                                                        unsigned             mask,
                                                        hyteg_hip_stream_t   stream );
/* the same restricted further to the edge-DoF orientations in kind_mask (bit 1..7 = X, Y, Z, XY, XZ, YZ, XYZ): the sweeps
 * "by type" of the P2 Gauss-Seidel smoother (sor_3D_macrocell_P2_update_edgedofs_by_type_*, P2ConstantOperator.cpp:913-1200) */
HYTEG_HIP_API int hyteg_hip_p2_edge_vector_cell_kinds( int                  op,
                                                       double*              dst,
                                                       int                  nsrc,
                                                       const double* const* srcs,
                                                       const double*        scalars,
                                                       int                  level,
                                                       unsigned             mask,
                                                       unsigned             kind_mask,
                                                       hyteg_hip_stream_t   stream );
HYTEG_HIP_API int hyteg_hip_p2_edge_dot_cell_masked( const double*      a,
                                                     const double*      b,
                                                     int                level,
                                                     unsigned           mask,
                                                     double*            result_dev,
                                                     void*              workspace_dev,
                                                     hyteg_hip_stream_t stream );
HYTEG_HIP_API int    hyteg_hip_p2_elementwise_apply_cell( double*            dst_vertex,
                                                          double*            dst_edge,
                                                          const double*      src_vertex,
                                                          const double*      src_edge,
                                                          int                level,
                                                          const double*      optable_dev,
                                                          double             alpha,
                                                          int                update,
                                                          unsigned           mask,
                                                          hyteg_hip_stream_t stream );
/* ... only the destination kinds in kind_mask (bit 0: vertex DoFs, 1..7: edge DoFs X, Y, Z, XY, XZ, YZ, XYZ) are computed and
 * written; the others are left alone */
HYTEG_HIP_API int    hyteg_hip_p2_elementwise_apply_cell_kinds( double*            dst_vertex,
                                                          double*            dst_edge,
                                                          const double*      src_vertex,
                                                          const double*      src_edge,
                                                          int                level,
                                                          const double*      optable_dev,
                                                          double             alpha,
                                                          int                update,
                                                          unsigned           mask,
                                                          unsigned           kind_mask,
                                                          hyteg_hip_stream_t stream );

/* The level from which hyteg_hip_p2_elementwise_apply_cell( .., kind mask 0xFF, mask with the inner DoFs ) uses the row kernel that
 * computes every point class (default 3, its lowest; 99 = never: the row kernel for the inner DoFs + the thread-per-DoF boundary kernel
 * of rounds 1-2).  Returns the previous value.  Results of the two agree to rounding (different partial sums), so this is a tuning and
 * test switch, not part of the operator interface (no reference counterpart). */
HYTEG_HIP_API int hyteg_hip_p2_set_class_rows_min_level( int level );

/* hyteg_hip_p2_edge_vector_cell_kinds for up to HYTEG_HIP_MAX_BATCH macro-cells of one level in ONE launch (the EdgeDoFFunction loops over
 * the macro-cells of a rank, src/hyteg/edgedofspace/EdgeDoFFunction.cpp): dst and masks are HOST arrays of ncells entries, srcs a HOST
 * array [nsrc][ncells] of device pointers */
HYTEG_HIP_API int hyteg_hip_p2_edge_vector_cells_kinds( int op, int ncells, double* const* dst, int nsrc, const double* const* srcs,
                                                        const double* scalars, int level, const unsigned* masks, unsigned kind_mask,
                                                        hyteg_hip_stream_t stream );

/* hyteg_hip_p2_edge_dot_cell_masked for up to HYTEG_HIP_MAX_BATCH macro-cells in one launch: results_dev[c] = the masked dot product of cell c
 * (a, b, masks: HOST arrays of ncells entries; one workgroup per cell, fixed summation order) */
HYTEG_HIP_API int hyteg_hip_p2_edge_dot_cells_masked( int ncells, const double* const* a, const double* const* b, int level, const unsigned* masks,
                                                      double* results_dev, hyteg_hip_stream_t stream );
/* hyteg_hip_p1_reduce_cells for the edge-DoF arrays (same arguments, results, workspace and guarantees; entries selected by point class
 * as in hyteg_hip_p2_edge_dot_cells_masked): the macro-cell loops of EdgeDoFFunction::sumLocal, getMaxDoFValue, getMinDoFValue and
 * getMaxDoFMagnitude (src/hyteg/edgedofspace/EdgeDoFFunction.cpp:1284-1490).  Levels 0..HYTEG_HIP_P2_MAX_LEVEL; up to 32 tiles of 256
 * entries (level 4) one workgroup per cell, above that up to 1024 per cell and a second launch. */
HYTEG_HIP_API int hyteg_hip_p2_edge_reduce_cells( int ncells, const double* const* a, int level, const unsigned* masks, double* results_dev,
                                                  void* workspace_dev, hyteg_hip_stream_t stream );
/* hyteg_hip_p2_elementwise_apply_cell_kinds for up to HYTEG_HIP_MAX_BATCH macro-cells of one level in two launches (inner DoFs, boundary
 * DoFs; P2ElementwiseOperator::gemv's loop over the macro-cells, P2ElementwiseOperator.cpp:131-223): all arguments per cell as HOST
 * arrays of ncells entries.  Levels 2..6 (thread-per-DoF kernels: where a launch per cell is pure launch latency). */
HYTEG_HIP_API int hyteg_hip_p2_elementwise_apply_cells_kinds( int ncells, double* const* dst_vertex, double* const* dst_edge, const double* const* src_vertex,
                                                              const double* const* src_edge, int level, const double* const* optables_dev, double alpha,
                                                              int update, const unsigned* masks, unsigned kind_mask, hyteg_hip_stream_t stream );

/* ---- P2 Gauss-Seidel / SOR on macro-primitives shared between macro-cells, in the reference's order ----
 * P2ConstantOperator::smooth_sor (src/constant_stencil_operator/P2ConstantOperator.cpp:1267-1330): macro-vertices (:157-201),
 * macro-edges (:205-266, P2MacroEdge.cpp:617-680), macro-faces (:269-880, kernels
 * P2generatedKernels/sor_3D_macroface_P2_update_{vertexdofs,edgedofs}*.cpp), macro-cells.  A primitive's sweep sees current
 * values on itself and on its boundary and ghost-layer values elsewhere.  Pieces for a cell-centric implementation:
 *  - hyteg_hip_p2_operator_table_closure_split (host arrays of hyteg_hip_p2_operator_table_size() doubles): splits the rows of
 *    the 14 boundary point classes of an operator table by where the SOURCE lies: `outside` keeps the weights of sources that do
 *    not lie on the closure of the destination's macro-primitive (what the reference reads from ghost layers), `closure_vertex` /
 *    `closure_edge` the weights of vertex- / edge-DoF sources on it.  Inner rows and element matrices are zero in all three:
 *    such tables serve the boundary classes at levels >= 2.
 *  - hyteg_hip_p2_operator_table_face_edge_weights: this cell's share of the couplings between the edge DoFs INSIDE one macro-face,
 *    in the face's own frame -- face_verts[3] = the cell-local vertex ids of the face's vertices in the order of their global ids
 *    (x runs from the first to the second, y from the first to the third); w[3][5]: for the face types X, XY, Y the diagonal
 *    and the four neighbours  X: XY(i,j) Y(i,j) XY(i,j-1) Y(i+1,j-1);  XY: X(i,j) Y(i,j) X(i,j+1) Y(i+1,j);
 *    Y: X(i,j) XY(i,j) X(i-1,j+1) XY(i-1,j)  (the other edges of the two face triangles that share the edge).
 *  - hyteg_hip_p2_sor_face_edgedofs_cell: sor_3D_macroface_P2_update_edgedofs[_backwards] on this cell's copy of its faces in
 *    `mask` (bits 6..9): rows ascending, x ascending, X, XY, Y at every index, each in place,
 *        u_i = (1 - relax) u_i + relax / w_ii ( q_i - sum_{in-face neighbours} w_ij u_j ),
 *    q = rhs - (everything that does not change during the sweep), face_w[4][3][5] = the TOTAL weights (sum of the shares of
 *    the cells at the face), face_verts[4][3] as above per face.  Every cell at a face runs the same sweep on its own copy.
 *    Levels 2..9. */
HYTEG_HIP_API int hyteg_hip_p2_operator_table_closure_split( const double* table_host, double* outside, double* closure_vertex, double* closure_edge );
HYTEG_HIP_API int hyteg_hip_p2_operator_table_face_edge_weights( const double* table_host, const int* face_verts /* 3 */, double* w /* 15 */ );
/* the same for up to HYTEG_HIP_MAX_BATCH macro-cells in one launch (levels 2..6): hyteg_hip_p2_sor_face_frames turns a cell's face_verts[4][3]
 * and face_w[4][3][5] into hyteg_hip_p2_sor_face_frames_bytes() bytes (host; a multiple of 8); the caller keeps the records of its cells, one
 * after the other, in device memory (frames_dev) */
HYTEG_HIP_API size_t hyteg_hip_p2_sor_face_frames_bytes( void );
HYTEG_HIP_API int    hyteg_hip_p2_sor_face_frames( int level, const int* face_verts /* 12 */, const double* face_w /* 60 */, void* frames_host );
HYTEG_HIP_API int    hyteg_hip_p2_sor_face_edgedofs_cells( int ncells, double* const* dst_edge, const double* const* q_edge, int level, const void* frames_dev,
                                                           double relax, const unsigned* masks, int backwards, hyteg_hip_stream_t stream );
HYTEG_HIP_API int hyteg_hip_p2_sor_face_edgedofs_cell( double* dst_edge, const double* q_edge, int level, const int* face_verts /* 12 */,
                                                       const double* face_w /* 60 */, double relax, unsigned mask, int backwards,
                                                       hyteg_hip_stream_t stream );

/* a10: additive exchange of shared points (the reduce-into-owner of VertexDoFAdditivePackInfo.hpp:676-745,
 * followed by the copy back into every adjacent cell).  A group is one physical DoF; its entries are the
 * places that hold a partial value of it: (buffer index into `bases`, element offset).
 *   out[e] = init + sum_{e in group} bases[buf_e][off_e]   in entry order (fixed, so every rank gets the same bits),
 * written back to every entry whose buffer index is < n_writable (local cell arrays; receive buffers follow).
 * All arrays are device memory except the scalars. */
HYTEG_HIP_API int hyteg_hip_sum_shared( double* const*     bases /* device table of device pointers */,
                                        const int*         group_ptr /* device, ngroups+1 */,
                                        const int*         entry_buf /* device, nentries */,
                                        const int*         entry_off /* device, nentries */,
                                        int                ngroups,
                                        int                n_writable,
                                        hyteg_hip_stream_t stream );
/* same groups, but every writable entry := the value of the group's FIRST entry (owner copy wins); used after
 * host-side interpolation, where the copies of a shared DoF may differ in the last bit */
HYTEG_HIP_API int hyteg_hip_copy_shared( double* const*     bases,
                                         const int*         group_ptr,
                                         const int*         entry_buf,
                                         const int*         entry_off,
                                         int                ngroups,
                                         int                n_writable,
                                         hyteg_hip_stream_t stream );
/* pack: out[k] = bases[buf[k]][off[k]]  (send buffer for one peer) */
HYTEG_HIP_API int hyteg_hip_gather_entries( double*            out,
                                            double* const*     bases,
                                            const int*         entry_buf,
                                            const int*         entry_off,
                                            int                n,
                                            hyteg_hip_stream_t stream );

/* ---- a9 / a10 in HyTeG's own macro-face layout (drop-in for the face seam) -----------------------------------
 * Macro-face array of width N = 2^level + 1:  [ tri(N) face DoFs | tri(N-1) ghost layer of neighbour cell 0 |
 * tri(N-1) ghost layer of neighbour cell 1 ]  (src/hyteg/p1functionspace/VertexDoFMemory.hpp:59-63,
 * VertexDoFIndexing.cpp:219-226).  v0,v1,v2 = cell.getFaceLocalVertexToCellLocalVertexMaps()[localFaceID], the
 * arguments of the reference's generated copy kernels.
 *
 * copy_face_to_cell replaces vertexdof::comm::generated::communicate_directly_vertexdof_face_to_cell
 *   (src/hyteg/p1functionspace/generatedKernels/communicate_directly_vertexdof_face_to_cell*.cpp; caller
 *    VertexDoFPackInfo.hpp:438-478): all tri(N) face DoFs onto the cell's boundary layer.
 * copy_cell_to_face replaces communicate_directly_vertexdof_cell_to_face (caller VertexDoFPackInfo.hpp:552-615):
 *   the cell layer at distance 1 from the face into ghost layer `neighbor` (the face's cell_index of that cell).
 * apply_face3d replaces apply_3D_macroface_one_sided_vertexdof_to_vertexdof_{replace,add} called once per
 *   neighbour cell (src/constant_stencil_operator/P1ConstantOperator.cpp:239-357; spec P1Operator.hpp:1111-1173):
 *   dst_i (=|+=) sum over the ncells (1 or 2) neighbour cells of that cell's share of the stencil.
 *   vmaps: host, ncells x 3; w: host, ncells x 15 weights in the CELL's stencil directions (w[15] order; entries
 *   for directions that leave the cell are ignored) -- faceStencil3D[cell] of the reference. */
HYTEG_HIP_API int hyteg_hip_p1_copy_face_to_cell( double* cell, const double* face, int level, int v0, int v1, int v2, hyteg_hip_stream_t stream );
HYTEG_HIP_API int hyteg_hip_p1_copy_cell_to_face( double* face, const double* cell, int level, int v0, int v1, int v2, int neighbor,
                                                  hyteg_hip_stream_t stream );
HYTEG_HIP_API int hyteg_hip_p1_apply_face3d( double*            dst_face,
                                             const double*      src_face,
                                             int                level,
                                             int                ncells,
                                             const int*         vmaps /* host, ncells*3 */,
                                             const double*      w /* host, ncells*15 */,
                                             int                update,
                                             hyteg_hip_stream_t stream );
/* sor_face3d replaces vertexdof::macroface::generated::sor_3D_macroface_P1 / _one_sided and their _backwards variants
 *   (src/constant_stencil_operator/P1generatedKernels/sor_3D_macroface_P1*.cpp; call site P1ConstantOperator.cpp:432-571;
 *   the loop they unroll: P1Operator::smooth_sor_face3D, P1Operator.hpp:1424-1503): in-place SOR / Gauss-Seidel sweep over
 *   the inner DoFs of ONE macro-face in lexicographic (y, x) order (backwards: reversed), ghost layers read as they are.
 *   dst_face: face array with ncells ghost layers; rhs_face: at least the tri(N) face DoFs; vmaps, w as for apply_face3d
 *   (w[7] of every cell = its share of the centre weight).  work: hyteg_hip_p1_sor_face3d_workspace( level ) bytes of
 *   device memory (the sweep is split into a parallel preparation pass and a wavefront pass; the values in between live
 *   there).  The updates are made in the reference's order; the terms of one update are summed in a different order
 *   (tests compare at 1e-12). */
HYTEG_HIP_API size_t hyteg_hip_p1_sor_face3d_workspace( int level );
HYTEG_HIP_API int hyteg_hip_p1_sor_face3d( double*            dst_face,
                                           const double*      rhs_face,
                                           double*            work,
                                           int                level,
                                           int                ncells,
                                           const int*         vmaps /* host, ncells*3 */,
                                           const double*      w /* host, ncells*15 */,
                                           double             relax,
                                           int                backwards,
                                           hyteg_hip_stream_t stream );

/* ---- f1: quadratic (P2) grid transfer on one macro-cell -----------------------------------------------------------
 * replaces P2toP2QuadraticProlongation::prolongateAdditively3D and P2toP2QuadraticRestriction::restrictAdditively3D
 *   src/hyteg/gridtransferoperators/P2toP2QuadraticProlongation.cpp:217-424,
 *   generatedKernels/prolongate_3D_macrocell_P2_push_from_{vertexdofs,edgedofs}.cpp
 *   src/hyteg/gridtransferoperators/P2toP2QuadraticRestriction.cpp:131-286,
 *   generatedKernels/restrict_3D_macrocell_P2_update_{vertexdofs,edgedofs}.cpp
 * vertex arrays: macro-cell layout of width 2^level + 1; edge arrays: hyteg_hip_p2_edge_array_size( level ) entries, seven
 * orientation blocks (X, Y, Z, XY, XZ, YZ, XYZ).  mask: 15-bit point-class mask of the DESTINATION DoFs (bits 0..13: the
 * macro-primitive slots edge0..5, face0..3, vertex0..3; bit 14: inside the cell), as for the elementwise apply.
 * prolongate: fine = (update == ADD ? fine : 0) + quadratic interpolant of the coarse function at the fine DoFs.  Every
 *   cell computes the complete value of the fine DoFs on its boundary (the interpolant is continuous), so the copies of
 *   several cells agree up to rounding; the host layer makes them bit-identical with a copy, not a sum.
 * restrict: coarse = P^T fine, where fine DoFs on a macro-primitive shared by nnc[slot] cells are scaled by 1 / nnc[slot]
 *   (nnc: host, 14 values in slot order, the numNeighborCells* arguments of the reference kernels); the additive exchange
 *   over the cells completes the coarse DoFs on shared primitives. */
HYTEG_HIP_API int hyteg_hip_p2_prolongate_cell( double*            fine_vertex,
                                                double*            fine_edge,
                                                const double*      coarse_vertex,
                                                const double*      coarse_edge,
                                                int                coarse_level,
                                                int                update,
                                                unsigned           mask,
                                                hyteg_hip_stream_t stream );
HYTEG_HIP_API int hyteg_hip_p2_restrict_cell( double*            coarse_vertex,
                                              double*            coarse_edge,
                                              const double*      fine_vertex,
                                              const double*      fine_edge,
                                              int                coarse_level,
                                              const double*      nnc /* host, 14 */,
                                              unsigned           mask,
                                              hyteg_hip_stream_t stream );
/* hyteg_hip_p2_restrict_cell for up to HYTEG_HIP_MAX_BATCH macro-cells of one level in ONE launch
 * (the loop over the macro-cells of P2toP2QuadraticRestriction::restrictAdditively3D, P2toP2QuadraticRestriction.cpp:131-286).
 * Pointer arrays and masks are HOST arrays of length ncells; nnc_inv_dev: device table [ncells][14] = 1 / numNeighborCells
 * in the slot order of hyteg_hip_p2_restrict_cell.  Bit-identical to the per-cell calls (same table, term order and fma
 * chain); a cell whose mask is 0 is skipped, its arrays are not touched.  Every argument is checked before any GPU work. */
HYTEG_HIP_API int hyteg_hip_p2_restrict_cells( int                  ncells,
                                               double* const*       coarse_vertex,
                                               double* const*       coarse_edge,
                                               const double* const* fine_vertex,
                                               const double* const* fine_edge,
                                               int                  coarse_level,
                                               const double*        nnc_inv_dev,
                                               const unsigned*      masks,
                                               hyteg_hip_stream_t   stream );
/* hyteg_hip_p2_prolongate_cell for a batch (P2toP2QuadraticProlongation.cpp:217-424) */
HYTEG_HIP_API int hyteg_hip_p2_prolongate_cells( int                  ncells,
                                                 double* const*       fine_vertex,
                                                 double* const*       fine_edge,
                                                 const double* const* coarse_vertex,
                                                 const double* const* coarse_edge,
                                                 int                  coarse_level,
                                                 int                  update,
                                                 const unsigned*      masks,
                                                 hyteg_hip_stream_t   stream );

/* ---- P1 <-> P2 conversion on the macro-cells of a rank ----------------------------------------------------------------
 * replaces the macro-cell loops of P1toP2Conversion and P2toP1Conversion
 *   src/hyteg/gridtransferoperators/P1toP2Conversion.cpp:28-149
 *   src/hyteg/gridtransferoperators/P2toP1Conversion.cpp:28-150
 * A P2 function of level L has the DoFs of a P1 function of level L + 1: the point ( X, Y, Z ) of the vertex array of level
 * L + 1 is the P2 DoF with logical index ( X / 2, Y / 2, Z / 2 ) whose kind the parities of ( X, Y, Z ) select -- (e,e,e) vertex,
 * (o,e,e) X, (e,o,e) Y, (e,e,o) Z, (o,o,e) XY, (o,e,o) XZ, (e,o,o) YZ, (o,o,o) XYZ.  The conversion is this permutation: values
 * are copied, never rounded.
 * p1: hyteg_hip_cell_size( p2_level + 1 ) entries; p2_vertex: hyteg_hip_cell_size( p2_level ); p2_edge:
 * hyteg_hip_p2_edge_array_size( p2_level ) in the seven-block order of the grid transfer above.  p2_level: 0..HYTEG_HIP_P2_MAX_LEVEL.
 * masks: 15-bit point-class masks of the DESTINATION DoFs, as for hyteg_hip_p2_prolongate_cells (a point and the P2 DoF on it
 * have the same class); a DoF whose class is not selected keeps its value, a cell whose mask is 0 is skipped.
 * Pointer arrays and masks are HOST arrays of 1 <= ncells <= HYTEG_HIP_MAX_BATCH entries; one launch per call, no table, no
 * allocation and no synchronisation, so the calls are legal while `stream` is being captured.  Every argument is checked
 * before any GPU work: EINVAL for a level or ncells out of range, a null pointer, or a p1 array that is the p2_vertex or
 * p2_edge array of the same cell. */
HYTEG_HIP_API int hyteg_hip_p1_to_p2_cells( int                  ncells,
                                            double* const*       p2_vertex,
                                            double* const*       p2_edge,
                                            const double* const* p1,
                                            int                  p2_level,
                                            const unsigned*      masks,
                                            hyteg_hip_stream_t   stream );
HYTEG_HIP_API int hyteg_hip_p2_to_p1_cells( int                  ncells,
                                            double* const*       p1,
                                            const double* const* p2_vertex,
                                            const double* const* p2_edge,
                                            int                  p2_level,
                                            const unsigned*      masks,
                                            hyteg_hip_stream_t   stream );
/* the same for one macro-cell: the batch of one */
HYTEG_HIP_API int hyteg_hip_p1_to_p2_cell( double* p2_vertex, double* p2_edge, const double* p1, int p2_level, unsigned mask, hyteg_hip_stream_t stream );
HYTEG_HIP_API int hyteg_hip_p2_to_p1_cell( double* p1, const double* p2_vertex, const double* p2_edge, int p2_level, unsigned mask, hyteg_hip_stream_t stream );

/* ---- events and the neighbour exchange over RCCL (xGMI) --------------------------------------------------------
 * One process per GPU.  Replaces, on this path, what the reference does through waLBerla's BufferSystem over MPI:
 *   src/hyteg/communication/BufferedCommunication.cpp:181-470   start/endCommunication: pack, Isend/Irecv, wait, unpack
 *   src/hyteg/p1functionspace/VertexDoFAdditivePackInfo.hpp:676-745   payloads of the additive exchange
 *   src/hyteg/p1functionspace/VertexDoFFunction.cpp:1710-1717   dotGlobal: allReduceInplace( SUM ) of one scalar
 * The message pattern is sparse neighbour point-to-point: hyteg_hip_comm_exchange is ONE group of ncclSend / ncclRecv
 * pairs (one per peer rank) enqueued on `stream`, no host synchronisation, no staging; the caller orders it against its
 * pack / reduce kernels with events.  librccl is resolved at run time (a copy the process already holds -- PyTorch
 * ships and loads its own -- is reused; HYTEG_HIP_RCCL_LIB overrides the search). */
HYTEG_HIP_API int hyteg_hip_event_create( hyteg_hip_event_t* event );
/* events that carry a device timestamp: elapsed_ms waits for `stop` and returns the time between the two (hipEventElapsedTime) */
HYTEG_HIP_API int hyteg_hip_event_create_timing( hyteg_hip_event_t* event );
HYTEG_HIP_API int hyteg_hip_event_elapsed_ms( hyteg_hip_event_t start, hyteg_hip_event_t stop, float* ms );
HYTEG_HIP_API int hyteg_hip_event_destroy( hyteg_hip_event_t event );
HYTEG_HIP_API int hyteg_hip_event_record( hyteg_hip_event_t event, hyteg_hip_stream_t stream );
HYTEG_HIP_API int hyteg_hip_stream_wait_event( hyteg_hip_stream_t stream, hyteg_hip_event_t event );

#define HYTEG_HIP_COMM_ID_BYTES 128 /* sizeof( ncclUniqueId ) */
typedef void* hyteg_hip_comm_t;
/* HYTEG_HIP_OK if librccl could be resolved; origin (optional) receives where it came from and its version code */
HYTEG_HIP_API int hyteg_hip_comm_available( char* origin, size_t buflen );
/* rank 0 creates the id and distributes its HYTEG_HIP_COMM_ID_BYTES bytes to all ranks by whatever means the
 * application has (MPI_Bcast in HyTeG, a torch.distributed store in bench.py) */
HYTEG_HIP_API int hyteg_hip_comm_unique_id( unsigned char* id );
/* collective over all ranks; binds the communicator to the calling thread's current device */
HYTEG_HIP_API int hyteg_hip_comm_create( hyteg_hip_comm_t* comm, int nranks, int rank, const unsigned char* id );
HYTEG_HIP_API int hyteg_hip_comm_destroy( hyteg_hip_comm_t comm );
/* send[ sum of send_count[0..k) ... ) goes to peers[k], recv[ sum of recv_count[0..k) ... ) comes from peers[k]
 * (device buffers, counts in doubles, host arrays of length npeers); stream-ordered.  A peer may be the calling rank
 * itself (loop-back inside the group; what the single-GPU tests use). */
HYTEG_HIP_API int hyteg_hip_comm_exchange( hyteg_hip_comm_t   comm,
                                           int                npeers,
                                           const int*         peers,
                                           const double*      send,
                                           const int*         send_count,
                                           double*            recv,
                                           const int*         recv_count,
                                           hyteg_hip_stream_t stream );
/* in-place sum over all ranks of n doubles in device memory; stream-ordered */
HYTEG_HIP_API int hyteg_hip_comm_allreduce_sum( hyteg_hip_comm_t comm, double* values, int n, hyteg_hip_stream_t stream );

/* ---- the same exchange peer to peer: stores into IPC-mapped arenas of the neighbour GPUs (comm_p2p.hip) -----------
 * Same reference semantics as hyteg_hip_comm_exchange (BufferedCommunication.cpp:181-470), no library call per exchange:
 * every rank creates one arena (uncached device memory), hands its HYTEG_HIP_P2P_HANDLE_BYTES handle to the other ranks
 * of the node (any channel; the handle is a plain byte string) and maps theirs.  Inside its arena a rank lays out, per
 * exchange plan and peer, two receive slots (used alternately, by sequence parity) and one 8-byte flag word; it tells
 * each peer where they are, and the peer describes them, as pointers into ITS mapping of that arena, in a
 * hyteg_hip_p2p_peer_t.  hyteg_hip_p2p_pack gathers n values like hyteg_hip_gather_entries and stores value k into slot
 * [seq & 1] of the peer whose segment [start, start + count) holds k, then writes seq to every peer's flag word;
 * hyteg_hip_p2p_wait enqueues a kernel that returns once the npeers flag words at flags[p * stride] (this rank's own
 * arena) have reached seq, or sets *status to 1 + p after timeout_ms (0: 20 s) -- it never spins unbounded.
 * Sequence numbers start at 1 and grow by one per exchange of a plan on both sides. */
#define HYTEG_HIP_P2P_HANDLE_BYTES 64 /* sizeof( hipIpcMemHandle_t ) */
typedef struct
{
   double*             slot[2]; /* receive slots of this rank's segment in the peer's arena (mapped here) */
   unsigned long long* flag;    /* this rank's flag word in the peer's arena (mapped here) */
   int                 start;   /* first index of the peer's segment in the send enumeration */
   int                 count;
} hyteg_hip_p2p_peer_t;
/* kind (optional) receives 0 uncached / 1 fine-grained / 2 default memory (env HYTEG_HIP_P2P_ARENA; default uncached) */
HYTEG_HIP_API int hyteg_hip_p2p_arena_create( size_t bytes, void** base, unsigned char* handle, int* kind );
HYTEG_HIP_API int hyteg_hip_p2p_arena_destroy( void* base );
HYTEG_HIP_API int hyteg_hip_p2p_arena_open( const unsigned char* handle, void** mapped );
HYTEG_HIP_API int hyteg_hip_p2p_arena_close( void* mapped );
/* peers: device array of npeers descriptors; counter: device word, zero before the first call, owned by the plan */
HYTEG_HIP_API int hyteg_hip_p2p_pack( const hyteg_hip_p2p_peer_t* peers,
                                      int                         npeers,
                                      double* const*              bases,
                                      const int*                  entry_buf,
                                      const int*                  entry_off,
                                      int                         n,
                                      unsigned long long          seq,
                                      unsigned*                   counter,
                                      hyteg_hip_stream_t          stream );
/* hyteg_hip_p1_apply_cell_boundary + hyteg_hip_p2p_pack in one launch, for a rank that owns ONE macro-cell: a shell point q
 * (the enumeration of the boundary kernel: q in [0, 4 tri(N)), face by face, row by row) whose share other ranks need stores it
 * into the peers' slots as entries send_list[ send_first[q] .. send_first[q+1] ) of the plan's send enumeration; the last
 * workgroup publishes seq.  send_first has 4 tri(N) + 1 entries.  Same values, bit for bit, as the two calls. */
HYTEG_HIP_API int hyteg_hip_p1_apply_cell_boundary_p2p( double*                     dst,
                                                        const double*               src,
                                                        int                         level,
                                                        const double*               w_slots /* host, 14 x 15 */,
                                                        unsigned                    mask,
                                                        int                         update,
                                                        const int*                  send_first,
                                                        const int*                  send_list,
                                                        const hyteg_hip_p2p_peer_t* peers,
                                                        int                         npeers,
                                                        unsigned long long          seq,
                                                        unsigned*                   counter,
                                                        hyteg_hip_stream_t          stream );
/* hyteg_hip_sum_shared ( additive != 0 ) / hyteg_hip_copy_shared whose workgroups first wait like hyteg_hip_p2p_wait: the
 * wait kernel and the reduce kernel of an exchange in one launch */
HYTEG_HIP_API int hyteg_hip_reduce_shared_after_p2p( double* const*            bases,
                                                     const int*                group_ptr,
                                                     const int*                entry_buf,
                                                     const int*                entry_off,
                                                     int                       ngroups,
                                                     int                       n_writable,
                                                     int                       additive,
                                                     const unsigned long long* flags,
                                                     int                       npeers,
                                                     int                       stride,
                                                     unsigned long long        seq,
                                                     unsigned*                 status,
                                                     unsigned                  timeout_ms,
                                                     hyteg_hip_stream_t        stream );
HYTEG_HIP_API int hyteg_hip_p2p_wait( const unsigned long long* flags,
                                      int                       npeers,
                                      int                       stride,
                                      unsigned long long        seq,
                                      unsigned*                 status,
                                      unsigned                  timeout_ms,
                                      hyteg_hip_stream_t        stream );

/* ---- f4: the constant-stencil P2 operator at its kernel seam -------------------------------------------------------------
 * P2ConstantOperator::apply (src/constant_stencil_operator/P2ConstantOperator.cpp:100-112) = four sub-operators whose
 * macro-cell kernels take stencil MAPS and update the macro-cell's INNER DoFs:
 *   vertex->vertex  hyteg_hip_p1_apply_cell (above)
 *   edge->vertex    apply_3D_macrocell_edgedof_to_vertexdof_{replace,add}( src X, XY, XYZ, XZ, Y, YZ, Z, dst vertex, e2vStencilMap, level )
 *                   src/hyteg/mixedoperators/EdgeDoFToVertexDoFOperator/generatedKernels/apply_3D_macrocell_edgedof_to_vertexdof_replace.hpp:36
 *   vertex->edge    apply_3D_macrocell_vertexdof_to_edgedof_{replace,add}( dst X, ..., Z, src vertex, level, v2eStencilMap )
 *                   src/hyteg/mixedoperators/VertexDoFToEdgeDoFOperator/generatedKernels/apply_3D_macrocell_vertexdof_to_edgedof_replace.hpp:36
 *   edge->edge      apply_3D_macrocell_edgedof_to_edgedof_{replace,add}( dst X, ..., Z, src X, ..., Z, e2eStencilMap, level )
 *                   src/constant_stencil_operator/EdgeDoFGeneratedKernels/apply_3D_macrocell_edgedof_to_edgedof_replace.hpp:37
 * The entry points keep the reference's pointer lists (the seven pointers must be the blocks of ONE edge-DoF array, which is
 * what the reference passes: &data[ index( level, 0, 0, 0, orientation ) ]) and take the stencil map's VALUES flattened in the
 * map's own iteration order -- orientations in the order of the enum (X, Y, Z, XY, XZ, YZ, XYZ), offsets in indexing::Index
 * order (z, y, x):
 *     for ( auto& a : e2eStencilMap ) for ( auto& b : a.second ) for ( auto& c : b.second ) w[k++] = c.second;
 * hyteg_hip_p2_constant_stencil_layout gives the number of values of the four maps (counts[4]: v2v, e2v, v2e, e2e) and, if
 * keys != NULL, for every value of the concatenation v2v | e2v | v2e | e2e the five integers { destination kind, source kind,
 * dx, dy, dz } (kind 0 = vertex DoFs, 1..7 = edge DoFs X, Y, Z, XY, XZ, YZ, XYZ; offset = source index - destination index),
 * so that a binding can check its maps' keys.  Levels 2..9.  These three calls run the fused kernel with all other weights
 * zero; the fast path is ONE pass for all four sub-operators: hyteg_hip_p2_build_operator_table_from_stencils turns the
 * concatenated values (inner DoFs) and, optionally, the cell's share stencils of the 14 boundary point classes
 * (classes[14][total], zero where a neighbour lies outside the cell) into the table hyteg_hip_p2_elementwise_apply_cell takes. */
HYTEG_HIP_API int hyteg_hip_p2_constant_stencil_layout( int* counts /* 4 */, int* keys /* NULL or 5 * total */ );
HYTEG_HIP_API int hyteg_hip_p2_build_operator_table_from_stencils( const double* inner /* total */, const double* classes /* NULL or 14 * total */,
                                                                   double* table_host );
HYTEG_HIP_API int hyteg_hip_p2_apply_cell_edgedof_to_vertexdof( const double* src_x, const double* src_xy, const double* src_xyz, const double* src_xz,
                                                                const double* src_y, const double* src_yz, const double* src_z, double* dst_vertex,
                                                                const double* e2v_stencil, int level, int update, hyteg_hip_stream_t stream );
HYTEG_HIP_API int hyteg_hip_p2_apply_cell_vertexdof_to_edgedof( double* dst_x, double* dst_xy, double* dst_xyz, double* dst_xz, double* dst_y,
                                                                double* dst_yz, double* dst_z, const double* src_vertex, int level,
                                                                const double* v2e_stencil, int update, hyteg_hip_stream_t stream );
HYTEG_HIP_API int hyteg_hip_p2_apply_cell_edgedof_to_edgedof( double* dst_x, double* dst_xy, double* dst_xyz, double* dst_xz, double* dst_y, double* dst_yz,
                                                              double* dst_z, const double* src_x, const double* src_xy, const double* src_xyz,
                                                              const double* src_xz, const double* src_y, const double* src_yz, const double* src_z,
                                                              const double* e2e_stencil, int level, int update, hyteg_hip_stream_t stream );

/* ---- b-3: the seam of the generated elementwise operators (module hyteg_operators) ---------------------------------------
 * The generated operators call, per macro-cell,
 *    apply_macro_3D( dst*, src*, macro_vertex_coord_id_{0..3}comp{0..2} (12 scalars), int64 micro_edges_per_macro_edge,
 *                    (value type) micro_edges_per_macro_edge_float )
 * (apps/2023-zikeli-mt/MT-apps/operators-used/P1ElementwiseDiffusion_cubes_const_float64.hpp:95-130, kernel .cpp:782-;
 * call site .cpp:76-165: halo synchronised and dst zeroed before, additive communication afterwards).  The entry points
 * below have that argument list (the twelve coordinates as one array [vertex][component]) and that effect:
 *    dst += ( operator of THIS macro-cell ) src   at ALL points of the cell array,
 * i.e. the full stencil at inner points and this cell's share at points on its macro-faces / -edges / -vertices.
 * The element matrices are computed on the host from the coordinates (constant per micro-cell type on an affine cell) and
 * summed into the constant stencils of the 15 point classes; results agree with the reference's element-by-element
 * scatter to rounding (the reference's own criterion for constant-stencil vs elementwise: < 1e-13,
 * tests/hyteg/convergence/P1JacobiConvergenceTest.cpp:117).  micro_edges_per_macro_edge = 2^level, levels 0..11
 * (float: 0..10). */
HYTEG_HIP_API int hyteg_hip_p1_elementwise_diffusion_apply_macro_3d( double*            dst,
                                                                     const double*      src,
                                                                     const double*      macro_vertex_coords /* 12: [vertex][component] */,
                                                                     int64_t            micro_edges_per_macro_edge,
                                                                     double             micro_edges_per_macro_edge_float,
                                                                     hyteg_hip_stream_t stream );
/* The same kernel restricted to the point classes of `mask` (as hyteg_hip_p1_apply_cell_boundary: bit k < 14 = points on slot k,
 * HYTEG_HIP_MASK_INNER = inner points) with REPLACE or ADD: for callers whose cell arrays hold the shared DoFs themselves (the
 * host layer here) instead of a halo that may be zeroed.  ( HYTEG_HIP_MASK_ALL, HYTEG_HIP_ADD ) is the call above. */
HYTEG_HIP_API int hyteg_hip_p1_elementwise_diffusion_apply_macro_3d_masked( double*            dst,
                                                                            const double*      src,
                                                                            const double*      macro_vertex_coords,
                                                                            int64_t            micro_edges_per_macro_edge,
                                                                            unsigned           mask,
                                                                            int                update,
                                                                            hyteg_hip_stream_t stream );
/* float32 sibling (P1ElementwiseDiffusion_cubes_const_float32.hpp); stencils are summed in double and rounded to float */
HYTEG_HIP_API int hyteg_hip_p1_elementwise_diffusion_apply_macro_3d_f32( float*             dst,
                                                                         const float*       src,
                                                                         const float*       macro_vertex_coords,
                                                                         int64_t            micro_edges_per_macro_edge,
                                                                         float              micro_edges_per_macro_edge_float,
                                                                         hyteg_hip_stream_t stream );
/* computeInverseDiagonalOperatorValues_macro_3D of the same operators: diag += the diagonal entries of the element matrices
 * of the adjacent micro-cells at all points of the cell array (levels 0..10) */
HYTEG_HIP_API int hyteg_hip_p1_elementwise_diffusion_diagonal_macro_3d( double*            diag,
                                                                        const double*      macro_vertex_coords,
                                                                        int64_t            micro_edges_per_macro_edge,
                                                                        double             micro_edges_per_macro_edge_float,
                                                                        hyteg_hip_stream_t stream );
/* host helper: the stencils the calls above use -- w_inner[15] and w_slots[14][15] in the conventions of
 * hyteg_hip_p1_apply_cell / hyteg_hip_p1_apply_cell_boundary */
HYTEG_HIP_API int hyteg_hip_p1_elementwise_diffusion_stencils( const double* macro_vertex_coords,
                                                               int64_t       micro_edges_per_macro_edge,
                                                               double*       w_inner,
                                                               double*       w_slots );
/* float instantiation of hyteg_hip_p1_apply_cell_boundary (used by the float seam above) */
HYTEG_HIP_API int hyteg_hip_p1_apply_cell_boundary_f32( float*             dst,
                                                        const float*       src,
                                                        int                level,
                                                        const double*      w_slots,
                                                        unsigned           mask,
                                                        int                update,
                                                        hyteg_hip_stream_t stream );
/* P2 form of the seam (generated P2ElementwiseDiffusion; its source is absent from the snapshot -- call sites
 * src/hyteg_operators_composites/viscousblock/P2ViscousBlockLaplaceOperator.hpp:29,66 -- so the ORDER of the four array
 * arguments is this header's convention, vertex before edge: parity unpinned for the argument order).
 * dst += A_cell src on all vertex and edge DoFs of the macro-cell; levels 0..9.  The six 10 x 10 element matrices
 * (FEniCS ordering, micro-cell types in the order of celldof::allCellTypes) are available through the second call. */
HYTEG_HIP_API int hyteg_hip_p2_elementwise_diffusion_apply_macro_3d( double*            dst_vertex,
                                                                     double*            dst_edge,
                                                                     const double*      src_vertex,
                                                                     const double*      src_edge,
                                                                     const double*      macro_vertex_coords,
                                                                     int64_t            micro_edges_per_macro_edge,
                                                                     double             micro_edges_per_macro_edge_float,
                                                                     hyteg_hip_stream_t stream );
HYTEG_HIP_API int hyteg_hip_p2_elementwise_diffusion_element_matrices( const double* macro_vertex_coords,
                                                                       int64_t       micro_edges_per_macro_edge,
                                                                       double*       elmat /* 600 */ );

/* ---- b-4: variable-coefficient diffusion -div( k grad u ), the seam of the generated P1ElementwiseDivKGrad ------------------
 * Replaces apply_macro_3D of operatorgeneration::P1ElementwiseDivKGrad( storage, minLevel, maxLevel, const P1Function< real_t >& k )
 * (module hyteg_operators; used in tests/hyteg/convergence/ElementwiseDivKGradCGConvergenceTest.cpp).  The generated source is
 * absent from the snapshot, so the ORDER of the array arguments (dst, src, k) is this header's convention (parity unpinned for
 * the argument order), and the arithmetic is pinned by the identity below, not by the generated code: with k a P1 function the
 * element matrix of micro-cell e is  mean( k at the 4 vertices of e ) * K_e,  K_e the P1 Laplace element matrix of e's type (a
 * generator may integrate with a rule of lower exactness and differ by rounding).  Per macro-cell semantics of
 * hyteg_hip_p1_elementwise_diffusion_apply_macro_3d_masked: at every point of the classes of `mask` the sum over the micro-cells
 * of THIS macro-cell that contain the point (24 at an inner point, this cell's share on the shell); entries outside the mask are
 * not written.  k: the coefficient's cell array at the same level.  Levels 0..8; dst must not alias src or k. */
HYTEG_HIP_API int hyteg_hip_p1_elementwise_divkgrad_apply_macro_3d_masked( double*            dst,
                                                                           const double*      src,
                                                                           const double*      k,
                                                                           const double*      macro_vertex_coords /* 12 */,
                                                                           int64_t            micro_edges_per_macro_edge,
                                                                           unsigned           mask,
                                                                           int                update,
                                                                           hyteg_hip_stream_t stream );
/* Fused form of P1ElementwiseOperator::smooth_jac (src/hyteg/elementwiseoperators/P1ElementwiseOperator.cpp:288-331: one apply
 * and three vector passes) for this operator, at the INNER points only:  dst = src + omega * inv_diag .* ( rhs - A src ).
 * dst must not alias an input.  Levels 0..8 (nothing to do below level 2). */
HYTEG_HIP_API int hyteg_hip_p1_elementwise_divkgrad_jacobi_macro_3d( double*            dst,
                                                                     const double*      src,
                                                                     const double*      rhs,
                                                                     const double*      inv_diag,
                                                                     const double*      k,
                                                                     const double*      macro_vertex_coords,
                                                                     int64_t            micro_edges_per_macro_edge,
                                                                     double             omega,
                                                                     hyteg_hip_stream_t stream );
/* Fused residual of a multigrid cycle for this operator, at the INNER points only:  dst = rhs - A src.  Replaces the apply and the
 * assign of GeometricMultigridSolver::solveRecursively (src/hyteg/solvers/GeometricMultigridSolver.hpp:240-246): one pass over the
 * arrays instead of two.  dst must alias neither src, rhs nor k, and neither input may be k (EINVAL).  Levels 0..8 (nothing to do
 * below level 2). */
HYTEG_HIP_API int hyteg_hip_p1_elementwise_divkgrad_residual_macro_3d( double*            dst,
                                                                       const double*      src,
                                                                       const double*      rhs,
                                                                       const double*      k,
                                                                       const double*      macro_vertex_coords,
                                                                       int64_t            micro_edges_per_macro_edge,
                                                                       hyteg_hip_stream_t stream );
/* The steps of ChebyshevSmoother::solve (src/hyteg/solvers/ChebyshevSmoother.hpp:165-212) for this operator, fused, at the INNER
 * points only, with the semantics of hyteg_hip_p1_chebyshev_start_cell / _step_cell above:
 *   start:  t_out = inv_diag .* ( rhs - A x );  x is the stencil source and is not updated (x += c_0 t_out is deferred to the next
 *           step, or to a vector pass for a smoother of order 1)
 *   step:   t_out = inv_diag .* ( A t_in ),  x = ( x + c_prev t_in ) + c_cur t_out, the first summand only if has_prev != 0; x is
 *           read and rewritten at the output points only.
 * A written array (t_out, x) must alias no other array of the call, and no array may be k (EINVAL).  Levels 0..8. */
HYTEG_HIP_API int hyteg_hip_p1_elementwise_divkgrad_chebyshev_start_macro_3d( double*            t_out,
                                                                              const double*      rhs,
                                                                              const double*      x,
                                                                              const double*      inv_diag,
                                                                              const double*      k,
                                                                              const double*      macro_vertex_coords,
                                                                              int64_t            micro_edges_per_macro_edge,
                                                                              hyteg_hip_stream_t stream );
HYTEG_HIP_API int hyteg_hip_p1_elementwise_divkgrad_chebyshev_step_macro_3d( double*            t_out,
                                                                             double*            x,
                                                                             const double*      t_in,
                                                                             const double*      inv_diag,
                                                                             const double*      k,
                                                                             const double*      macro_vertex_coords,
                                                                             int64_t            micro_edges_per_macro_edge,
                                                                             double             c_prev,
                                                                             double             c_cur,
                                                                             int                has_prev,
                                                                             hyteg_hip_stream_t stream );
/* Replaces computeInverseDiagonalOperatorValues_macro_3D of the same class: diag += sum over the adjacent micro-cells e of this
 * macro-cell of mean_k( e ) * K_e[i,i], at all points of the cell array. */
HYTEG_HIP_API int hyteg_hip_p1_elementwise_divkgrad_diagonal_macro_3d( double*            diag,
                                                                       const double*      k,
                                                                       const double*      macro_vertex_coords,
                                                                       int64_t            micro_edges_per_macro_edge,
                                                                       hyteg_hip_stream_t stream );
/* Tuning knobs of the kernels above (no counterpart in the reference): the brick shape of the inner-point z-march (rows x slices
 * per wave; 0, 0 = the default of the level; EINVAL for a shape that is not compiled in), and the inner points by the
 * one-thread-per-point kernel instead (the form the z-march is measured against).  Every choice computes the same bits. */
HYTEG_HIP_API int hyteg_hip_p1_elementwise_divkgrad_set_shape( int ny, int lz );
HYTEG_HIP_API int hyteg_hip_p1_elementwise_divkgrad_set_inner_by_points( int on );

/* ---- b-4 (P2): -div( k grad u ) on P2 with a P2 coefficient, the seam of the generated P2ElementwiseDivKGrad ----------------
 * Replaces operatorgeneration::P2ElementwiseDivKGrad::apply of operatorgeneration::P2ElementwiseDivKGrad( storage, minLevel, maxLevel,
 * const P2Function< real_t >& k ) (module hyteg_operators; in-tree use: tests/hyteg/convergence/ElementwiseDivKGradCGConvergenceTest.cpp:
 * 192-221, runAllTestsP2).  The generated source is absent from the snapshot, so the arithmetic is pinned by the identity, not by the
 * generated code: on a micro-cell e,  A_e[i][j] = sum_m k_m int_e phi_m grad phi_i . grad phi_j  over the ten DoFs m of e, integrated
 * exactly (degree 4; forms::p2_div_k_grad_affine_q4 evaluates the same form with a degree-4 rule), local DoFs in the FEniCS order of
 * P2Form::integrateAll.  Arrays, alpha, update, the 15-bit point-class mask and the 8-bit kind_mask are those of
 * hyteg_hip_p2_elementwise_apply_cell_kinds (7-block edge array, XYZ block of tet( 2^level - 1 )); k_vertex / k_edge: the coefficient's
 * arrays at the same level; entries outside mask and kinds are not written.  Levels 0..8 (32-bit indices).
 * EINVAL before any GPU work: a level out of range, a null array, a written array that is a src or k array, a bad update type.
 *
 * hyteg_hip_p2_elementwise_divkgrad_geometry fills the 60 doubles the kernels need of a ( macro-cell, level ): |e| grad l_a . grad l_b / 840
 * of the six micro-cell types (pairs a <= b: 00 01 02 03 11 12 13 22 23 33); a HOST array, passed to the kernels in their arguments. */
HYTEG_HIP_API int hyteg_hip_p2_elementwise_divkgrad_geometry( const double* macro_vertex_coords /* 12 */, int level, double* geometry /* 60 */ );
/* Replaces operatorgeneration::P2ElementwiseDivKGrad::apply on one macro-cell (test file above).  Inner DoFs: the inner form
 * (compile-time micro-cell lists) from the level of hyteg_hip_p2_elementwise_divkgrad_set_inner_min_level on (default 6, where it
 * measures faster), below it the gather form; boundary DoFs of every level: the gather form. */
HYTEG_HIP_API int hyteg_hip_p2_elementwise_divkgrad_apply_cell_kinds( double*            dst_vertex,
                                                                      double*            dst_edge,
                                                                      const double*      src_vertex,
                                                                      const double*      src_edge,
                                                                      const double*      k_vertex,
                                                                      const double*      k_edge,
                                                                      int                level,
                                                                      const double*      geometry /* 60, host */,
                                                                      double             alpha,
                                                                      int                update,
                                                                      unsigned           mask,
                                                                      unsigned           kind_mask,
                                                                      hyteg_hip_stream_t stream );
/* The same operator (operatorgeneration::P2ElementwiseDivKGrad::apply, test file above) through the gather form on every DoF: the
 * second implementation the inner form is tested and measured against. */
HYTEG_HIP_API int hyteg_hip_p2_elementwise_divkgrad_apply_cell_gather( double*            dst_vertex,
                                                                       double*            dst_edge,
                                                                       const double*      src_vertex,
                                                                       const double*      src_edge,
                                                                       const double*      k_vertex,
                                                                       const double*      k_edge,
                                                                       int                level,
                                                                       const double*      geometry /* 60, host */,
                                                                       double             alpha,
                                                                       int                update,
                                                                       unsigned           mask,
                                                                       unsigned           kind_mask,
                                                                       hyteg_hip_stream_t stream );
/* Replaces the macro-cell part of operatorgeneration::P2ElementwiseDivKGrad::computeInverseDiagonalOperatorValues (test file above,
 * through the smoothers): every DoF of the cell receives the sum of A_e[i][i] over its adjacent micro-cells of THIS macro-cell
 * (Replace); the caller sums the shared copies and inverts.  diag arrays must not be k arrays. */
HYTEG_HIP_API int hyteg_hip_p2_elementwise_divkgrad_diagonal_cell( double*            diag_vertex,
                                                                   double*            diag_edge,
                                                                   const double*      k_vertex,
                                                                   const double*      k_edge,
                                                                   int                level,
                                                                   const double*      geometry /* 60, host */,
                                                                   hyteg_hip_stream_t stream );
/* Tuning knob of operatorgeneration::P2ElementwiseDivKGrad::apply above (no counterpart in the reference; test file above): the first
 * level whose inner DoFs take the inner form (at least 2; 99: the gather form everywhere).  Returns the previous value.
 * hyteg_hip_p2_elementwise_divkgrad_max_level: the largest level of these entries. */
HYTEG_HIP_API int hyteg_hip_p2_elementwise_divkgrad_set_inner_min_level( int level );
HYTEG_HIP_API int hyteg_hip_p2_elementwise_divkgrad_max_level( void );

/* b-4 (P2), fused modes: in the kernels of hyteg_hip_p2_elementwise_divkgrad_apply_cell_kinds every DoF holds its complete ( A src )
 * at the store; these entries replace the store by the arithmetic that follows the apply in the reference, read at the DoF's own index:
 *   residual          dst = rhs - A src: the apply and the assign of GeometricMultigridSolver::solveRecursively
 *                     (src/hyteg/solvers/GeometricMultigridSolver.hpp:240-246) on operatorgeneration::P2ElementwiseDivKGrad
 *   jacobi            dst = src + relax invdiag ( rhs - A src ): P2ElementwiseOperator::smooth_jac
 *                     (src/hyteg/elementwiseoperators/P2ElementwiseOperator.cpp:344-374) as its four statements (the last
 *                     multiply-add may contract to an FMA)
 *   chebyshev_start   t_out = invdiag ( rhs - A x ) and
 *   chebyshev_step    t_out = invdiag ( A t_in ), x = ( x + c_prev t_in ) + c_cur t_out (the first summand only if has_prev != 0): the
 *                     steps of ChebyshevSmoother::solve (src/hyteg/solvers/ChebyshevSmoother.hpp:165-212) with the semantics of
 *                     hyteg_hip_p1_chebyshev_start_cell / hyteg_hip_p1_chebyshev_step_cell, the deferred x += c_0 t after a start
 *                     included; x is read and written at the DoF's own index only and is not a source of the operator.
 * Arrays, level, geometry, mask and kind_mask as in apply_cell_kinds (alpha = 1, Replace); invdiag: the inverse diagonal's arrays.  A
 * DoF outside mask or kind_mask is written in no output array (t_out and x alike).  The shell / inner split and
 * hyteg_hip_p2_elementwise_divkgrad_set_inner_min_level act as in apply_cell_kinds; the _gather entries run the gather form on every DoF
 * (the second implementation).  EINVAL before any GPU work: a null array, a level outside 0..8, a written array (dst, t_out, x) that is
 * another array of the call, any array that is a k array.  An empty mask or kind_mask returns OK. */
HYTEG_HIP_API int hyteg_hip_p2_elementwise_divkgrad_residual_cell( double* dst_vertex, double* dst_edge, const double* src_vertex,
                                                                   const double* src_edge, const double* rhs_vertex, const double* rhs_edge,
                                                                   const double* k_vertex, const double* k_edge, int level,
                                                                   const double* geometry /* 60, host */, unsigned mask, unsigned kind_mask,
                                                                   hyteg_hip_stream_t stream );
HYTEG_HIP_API int hyteg_hip_p2_elementwise_divkgrad_residual_cell_gather( double* dst_vertex, double* dst_edge, const double* src_vertex,
                                                                          const double* src_edge, const double* rhs_vertex,
                                                                          const double* rhs_edge, const double* k_vertex, const double* k_edge,
                                                                          int level, const double* geometry /* 60, host */, unsigned mask,
                                                                          unsigned kind_mask, hyteg_hip_stream_t stream );
HYTEG_HIP_API int hyteg_hip_p2_elementwise_divkgrad_jacobi_cell( double* dst_vertex, double* dst_edge, const double* src_vertex,
                                                                 const double* src_edge, const double* rhs_vertex, const double* rhs_edge,
                                                                 const double* invdiag_vertex, const double* invdiag_edge,
                                                                 const double* k_vertex, const double* k_edge, int level,
                                                                 const double* geometry /* 60, host */, double relax, unsigned mask,
                                                                 unsigned kind_mask, hyteg_hip_stream_t stream );
HYTEG_HIP_API int hyteg_hip_p2_elementwise_divkgrad_jacobi_cell_gather( double* dst_vertex, double* dst_edge, const double* src_vertex,
                                                                        const double* src_edge, const double* rhs_vertex,
                                                                        const double* rhs_edge, const double* invdiag_vertex,
                                                                        const double* invdiag_edge, const double* k_vertex,
                                                                        const double* k_edge, int level, const double* geometry /* 60, host */,
                                                                        double relax, unsigned mask, unsigned kind_mask,
                                                                        hyteg_hip_stream_t stream );
HYTEG_HIP_API int hyteg_hip_p2_elementwise_divkgrad_chebyshev_start_cell( double* t_out_vertex, double* t_out_edge, const double* x_vertex,
                                                                          const double* x_edge, const double* rhs_vertex,
                                                                          const double* rhs_edge, const double* invdiag_vertex,
                                                                          const double* invdiag_edge, const double* k_vertex,
                                                                          const double* k_edge, int level, const double* geometry /* 60, host */,
                                                                          unsigned mask, unsigned kind_mask, hyteg_hip_stream_t stream );
HYTEG_HIP_API int hyteg_hip_p2_elementwise_divkgrad_chebyshev_start_cell_gather( double* t_out_vertex, double* t_out_edge,
                                                                                 const double* x_vertex, const double* x_edge,
                                                                                 const double* rhs_vertex, const double* rhs_edge,
                                                                                 const double* invdiag_vertex, const double* invdiag_edge,
                                                                                 const double* k_vertex, const double* k_edge, int level,
                                                                                 const double* geometry /* 60, host */, unsigned mask,
                                                                                 unsigned kind_mask, hyteg_hip_stream_t stream );
HYTEG_HIP_API int hyteg_hip_p2_elementwise_divkgrad_chebyshev_step_cell( double* t_out_vertex, double* t_out_edge, double* x_vertex,
                                                                         double* x_edge, const double* t_in_vertex, const double* t_in_edge,
                                                                         const double* invdiag_vertex, const double* invdiag_edge,
                                                                         const double* k_vertex, const double* k_edge, int level,
                                                                         const double* geometry /* 60, host */, double c_prev, double c_cur,
                                                                         int has_prev, unsigned mask, unsigned kind_mask,
                                                                         hyteg_hip_stream_t stream );
HYTEG_HIP_API int hyteg_hip_p2_elementwise_divkgrad_chebyshev_step_cell_gather( double* t_out_vertex, double* t_out_edge, double* x_vertex,
                                                                                double* x_edge, const double* t_in_vertex,
                                                                                const double* t_in_edge, const double* invdiag_vertex,
                                                                                const double* invdiag_edge, const double* k_vertex,
                                                                                const double* k_edge, int level,
                                                                                const double* geometry /* 60, host */, double c_prev,
                                                                                double c_cur, int has_prev, unsigned mask, unsigned kind_mask,
                                                                                hyteg_hip_stream_t stream );

/* ---- b-4 (P2 epsilon): variable-viscosity epsilon operator -div( 2 mu eps(u) ) on P2 with a P2 viscosity -----------------------
 * Replaces, in ONE pass over the three velocity components, the nine P2 elementwise block applies of
 * operatorgeneration::P2ViscousBlockEpsilonOperator::apply (module hyteg_operators; the velocity block of
 * operatorgeneration::P2P1StokesEpsilonOperator, which the reference's convection apps instantiate; for mu = 1 the in-tree
 * P2ElementwiseAffineEpsilonOperator of tests/hyteg/convergence/ElementwiseEpsilonMinResConvergenceTest.cpp:156-163, 366-412 and
 * src/mixed_operator/P2P1ElementwiseAffineEpsilonStokesOperator.hpp:61-70).  The generated source is absent from the snapshot, so the
 * arithmetic is pinned by the identity: on a micro-cell e, block ( i, j ) of the element matrix is
 * int_e mu ( delta_ij grad phi_b . grad phi_a + d_j phi_a d_i phi_b ), mu the P2 interpolant of its ten values on e, integrated exactly
 * (degree 4), local DoFs in the FEniCS order of P2Form::integrateAll.  dst_* / src_*: HOST arrays of three device pointers (the
 * components' vertex arrays and 7-block edge arrays as in hyteg_hip_p2_elementwise_apply_cell_kinds); mu_vertex / mu_edge: the viscosity's
 * arrays at the same level; mask[3]: a 15-bit point-class mask per destination component (the components of a P2VectorFunction may carry
 * different boundary conditions: a DoF that mask[i] excludes is not written in component i); kind_mask: the 8 destination kinds.
 * Levels 0..8 (32-bit indices).  EINVAL before any GPU work: a level out of range, a null array, a written array that is a src, mu or
 * another written array, a bad update type.
 *
 * hyteg_hip_p2_elementwise_epsilon_geometry fills the 72 doubles the kernels need of a ( macro-cell, level ):
 * sqrt( |e| / 840 ) d_r l_a of the six micro-cell types at [12 t + 3 a + r]; a HOST array, passed to the kernels in their arguments. */
HYTEG_HIP_API int hyteg_hip_p2_elementwise_epsilon_geometry( const double* macro_vertex_coords /* 12 */, int level, double* geometry /* 72 */ );
/* Replaces operatorgeneration::P2ViscousBlockEpsilonOperator::apply on one macro-cell (test file above).  Inner DoFs: the inner form
 * (compile-time micro-cell lists) from the level of hyteg_hip_p2_elementwise_epsilon_set_inner_min_level on, below it the gather form;
 * boundary DoFs of every level: the gather form. */
HYTEG_HIP_API int hyteg_hip_p2_elementwise_epsilon_apply_cell_kinds( double* const*       dst_vertex /* 3 */,
                                                                     double* const*       dst_edge /* 3 */,
                                                                     const double* const* src_vertex /* 3 */,
                                                                     const double* const* src_edge /* 3 */,
                                                                     const double*        mu_vertex,
                                                                     const double*        mu_edge,
                                                                     const unsigned*      mask /* 3 */,
                                                                     int                  level,
                                                                     const double*        geometry /* 72, host */,
                                                                     double               alpha,
                                                                     int                  update,
                                                                     unsigned             kind_mask,
                                                                     hyteg_hip_stream_t   stream );
/* The same operator (operatorgeneration::P2ViscousBlockEpsilonOperator::apply, test file above) through the gather form on every DoF:
 * the second implementation the inner form is tested and measured against. */
HYTEG_HIP_API int hyteg_hip_p2_elementwise_epsilon_apply_cell_gather( double* const*       dst_vertex /* 3 */,
                                                                      double* const*       dst_edge /* 3 */,
                                                                      const double* const* src_vertex /* 3 */,
                                                                      const double* const* src_edge /* 3 */,
                                                                      const double*        mu_vertex,
                                                                      const double*        mu_edge,
                                                                      const unsigned*      mask /* 3 */,
                                                                      int                  level,
                                                                      const double*        geometry /* 72, host */,
                                                                      double               alpha,
                                                                      int                  update,
                                                                      unsigned             kind_mask,
                                                                      hyteg_hip_stream_t   stream );
/* Replaces the macro-cell part of operatorgeneration::P2ViscousBlockEpsilonOperator::computeInverseDiagonalOperatorValues (the inverse
 * diagonals of the three diagonal blocks, test file above through the smoothers): component i of every DoF of the cell receives the sum
 * of A_e^{ii}[row][row] over its adjacent micro-cells of THIS macro-cell (Replace); the caller sums the shared copies and inverts.  diag
 * arrays must not be mu arrays. */
HYTEG_HIP_API int hyteg_hip_p2_elementwise_epsilon_diagonal_cell( double* const*     diag_vertex /* 3 */,
                                                                  double* const*     diag_edge /* 3 */,
                                                                  const double*      mu_vertex,
                                                                  const double*      mu_edge,
                                                                  int                level,
                                                                  const double*      geometry /* 72, host */,
                                                                  hyteg_hip_stream_t stream );
/* Tuning knob of operatorgeneration::P2ViscousBlockEpsilonOperator::apply above (no counterpart in the reference; test file above): the
 * first level whose inner DoFs take the inner form (at least 2; 99: the gather form everywhere).  Returns the previous value.
 * hyteg_hip_p2_elementwise_epsilon_max_level: the largest level of these entries. */
HYTEG_HIP_API int hyteg_hip_p2_elementwise_epsilon_set_inner_min_level( int level );
HYTEG_HIP_API int hyteg_hip_p2_elementwise_epsilon_max_level( void );

/* b-4 (P2 epsilon), fused modes: in the kernels of hyteg_hip_p2_elementwise_epsilon_apply_cell_kinds every DoF holds the complete
 * ( A src )_j of its three components at the store; these entries replace the store by the arithmetic that follows the apply in the
 * reference, read at the DoF's own index:
 *   residual          dst = rhs - A src: the apply and the assign of GeometricMultigridSolver::solveRecursively
 *                     (src/hyteg/solvers/GeometricMultigridSolver.hpp:240-246) on operatorgeneration::P2ViscousBlockEpsilonOperator
 *   jacobi            dst = src + relax invdiag ( rhs - A src ): P2ElementwiseOperator::smooth_jac
 *                     (src/hyteg/elementwiseoperators/P2ElementwiseOperator.cpp:344-374) per component as its four statements (the
 *                     last multiply-add may contract to an FMA)
 *   chebyshev_start   t_out = invdiag ( rhs - A x ) and
 *   chebyshev_step    t_out = invdiag ( A t_in ), x = ( x + c_prev t_in ) + c_cur t_out (the first summand only if has_prev != 0): the
 *                     steps of ChebyshevSmoother::solve (src/hyteg/solvers/ChebyshevSmoother.hpp:165-212) with the semantics of
 *                     hyteg_hip_p1_chebyshev_start_cell / hyteg_hip_p1_chebyshev_step_cell, the deferred x += c_0 t after a start
 *                     included; x is read and written at the DoF's own index only and is not a source of the operator.
 * Every array argument but mu is a HOST array of three device pointers; level, geometry, mask[3] and kind_mask as in apply_cell_kinds
 * (alpha = 1, Replace); invdiag: the inverse diagonals of the three diagonal blocks.  mask[i] = 0 switches component i off; a DoF that
 * mask[i] or kind_mask excludes is written in no output array of component i (t_out and x alike).  The shell / inner split and
 * hyteg_hip_p2_elementwise_epsilon_set_inner_min_level act as in apply_cell_kinds; the _gather entries run the gather form on every DoF
 * (the second implementation).  EINVAL before any GPU work: a null array, a level outside 0..8, a written array (dst, t_out, x) that is
 * another array of the call, any array that is a mu array.  Empty masks or an empty kind_mask return OK. */
HYTEG_HIP_API int hyteg_hip_p2_elementwise_epsilon_residual_cell( double* const* dst_vertex /* 3 */, double* const* dst_edge /* 3 */,
                                                                  const double* const* src_vertex /* 3 */, const double* const* src_edge /* 3 */,
                                                                  const double* const* rhs_vertex /* 3 */, const double* const* rhs_edge /* 3 */,
                                                                  const double* mu_vertex, const double* mu_edge, const unsigned* mask /* 3 */,
                                                                  int level, const double* geometry /* 72, host */, unsigned kind_mask,
                                                                  hyteg_hip_stream_t stream );
HYTEG_HIP_API int hyteg_hip_p2_elementwise_epsilon_residual_cell_gather( double* const* dst_vertex /* 3 */, double* const* dst_edge /* 3 */,
                                                                         const double* const* src_vertex /* 3 */,
                                                                         const double* const* src_edge /* 3 */,
                                                                         const double* const* rhs_vertex /* 3 */,
                                                                         const double* const* rhs_edge /* 3 */, const double* mu_vertex,
                                                                         const double* mu_edge, const unsigned* mask /* 3 */, int level,
                                                                         const double* geometry /* 72, host */, unsigned kind_mask,
                                                                         hyteg_hip_stream_t stream );
HYTEG_HIP_API int hyteg_hip_p2_elementwise_epsilon_jacobi_cell( double* const* dst_vertex /* 3 */, double* const* dst_edge /* 3 */,
                                                                const double* const* src_vertex /* 3 */, const double* const* src_edge /* 3 */,
                                                                const double* const* rhs_vertex /* 3 */, const double* const* rhs_edge /* 3 */,
                                                                const double* const* invdiag_vertex /* 3 */,
                                                                const double* const* invdiag_edge /* 3 */, const double* mu_vertex,
                                                                const double* mu_edge, const unsigned* mask /* 3 */, int level,
                                                                const double* geometry /* 72, host */, double relax, unsigned kind_mask,
                                                                hyteg_hip_stream_t stream );
HYTEG_HIP_API int hyteg_hip_p2_elementwise_epsilon_jacobi_cell_gather( double* const* dst_vertex /* 3 */, double* const* dst_edge /* 3 */,
                                                                       const double* const* src_vertex /* 3 */,
                                                                       const double* const* src_edge /* 3 */,
                                                                       const double* const* rhs_vertex /* 3 */,
                                                                       const double* const* rhs_edge /* 3 */,
                                                                       const double* const* invdiag_vertex /* 3 */,
                                                                       const double* const* invdiag_edge /* 3 */, const double* mu_vertex,
                                                                       const double* mu_edge, const unsigned* mask /* 3 */, int level,
                                                                       const double* geometry /* 72, host */, double relax, unsigned kind_mask,
                                                                       hyteg_hip_stream_t stream );
HYTEG_HIP_API int hyteg_hip_p2_elementwise_epsilon_chebyshev_start_cell( double* const* t_out_vertex /* 3 */, double* const* t_out_edge /* 3 */,
                                                                         const double* const* x_vertex /* 3 */,
                                                                         const double* const* x_edge /* 3 */,
                                                                         const double* const* rhs_vertex /* 3 */,
                                                                         const double* const* rhs_edge /* 3 */,
                                                                         const double* const* invdiag_vertex /* 3 */,
                                                                         const double* const* invdiag_edge /* 3 */, const double* mu_vertex,
                                                                         const double* mu_edge, const unsigned* mask /* 3 */, int level,
                                                                         const double* geometry /* 72, host */, unsigned kind_mask,
                                                                         hyteg_hip_stream_t stream );
HYTEG_HIP_API int hyteg_hip_p2_elementwise_epsilon_chebyshev_start_cell_gather( double* const* t_out_vertex /* 3 */,
                                                                                double* const* t_out_edge /* 3 */,
                                                                                const double* const* x_vertex /* 3 */,
                                                                                const double* const* x_edge /* 3 */,
                                                                                const double* const* rhs_vertex /* 3 */,
                                                                                const double* const* rhs_edge /* 3 */,
                                                                                const double* const* invdiag_vertex /* 3 */,
                                                                                const double* const* invdiag_edge /* 3 */,
                                                                                const double* mu_vertex, const double* mu_edge,
                                                                                const unsigned* mask /* 3 */, int level,
                                                                                const double* geometry /* 72, host */, unsigned kind_mask,
                                                                                hyteg_hip_stream_t stream );
HYTEG_HIP_API int hyteg_hip_p2_elementwise_epsilon_chebyshev_step_cell( double* const* t_out_vertex /* 3 */, double* const* t_out_edge /* 3 */,
                                                                        double* const* x_vertex /* 3 */, double* const* x_edge /* 3 */,
                                                                        const double* const* t_in_vertex /* 3 */,
                                                                        const double* const* t_in_edge /* 3 */,
                                                                        const double* const* invdiag_vertex /* 3 */,
                                                                        const double* const* invdiag_edge /* 3 */, const double* mu_vertex,
                                                                        const double* mu_edge, const unsigned* mask /* 3 */, int level,
                                                                        const double* geometry /* 72, host */, double c_prev, double c_cur,
                                                                        int has_prev, unsigned kind_mask, hyteg_hip_stream_t stream );
HYTEG_HIP_API int hyteg_hip_p2_elementwise_epsilon_chebyshev_step_cell_gather( double* const* t_out_vertex /* 3 */,
                                                                               double* const* t_out_edge /* 3 */,
                                                                               double* const* x_vertex /* 3 */, double* const* x_edge /* 3 */,
                                                                               const double* const* t_in_vertex /* 3 */,
                                                                               const double* const* t_in_edge /* 3 */,
                                                                               const double* const* invdiag_vertex /* 3 */,
                                                                               const double* const* invdiag_edge /* 3 */,
                                                                               const double* mu_vertex, const double* mu_edge,
                                                                               const unsigned* mask /* 3 */, int level,
                                                                               const double* geometry /* 72, host */, double c_prev,
                                                                               double c_cur, int has_prev, unsigned kind_mask,
                                                                               hyteg_hip_stream_t stream );

/* ---- b-5: variable-viscosity epsilon operator -div( 2 mu eps(u) ), eps(u) = ( grad u + grad u^T ) / 2 ------------------------
 * Replaces, in ONE pass over the three velocity components, the nine P1ElementwiseOperator::apply calls of
 * P1ElementwiseAffineEpsilonOperator::apply (src/mixed_operator/P1EpsilonOperator.hpp:89-164; forms::p1_epsilonvar_i_j_affine_q2)
 * on one macro-cell.  The viscosity is a P1 function (its cell array `mu` at the same level), where the reference samples a
 * std::function at the points of a degree-2 rule; the two coincide where mu is linear per micro-cell.  With constant barycentric
 * gradients g_a the block for test component i and trial component j of micro-cell e is exact and closed:
 *    A_e^{ij}[a][b] = mean( mu at the 4 vertices of e ) * |e| * ( delta_ij g_a . g_b + g_a[j] g_b[i] ).
 * dst, src: HOST arrays of three device pointers (the cell arrays of the components).  Semantics per macro-cell as in b-4: at every
 * point of the classes of `mask` the sum over the micro-cells of THIS macro-cell that contain the point; entries outside the mask
 * are not written.  Levels 0..8; no dst may alias a src, mu or another dst. */
HYTEG_HIP_API int hyteg_hip_p1_elementwise_epsilon_apply_macro_3d_masked( double* const*       dst /* 3 */,
                                                                          const double* const* src /* 3 */,
                                                                          const double*        mu,
                                                                          const double*        macro_vertex_coords /* 12 */,
                                                                          int64_t              micro_edges_per_macro_edge,
                                                                          unsigned             mask,
                                                                          int                  update,
                                                                          hyteg_hip_stream_t   stream );
/* The same with a class mask per destination component (masks[3]): the components of a P1VectorFunction may carry different
 * boundary conditions (P1EpsilonOperator.hpp applies block (i, j) with the flag on dst component i); a point that masks[i]
 * excludes is not written in dst[i].  One launch per kernel kind for all three components. */
HYTEG_HIP_API int hyteg_hip_p1_elementwise_epsilon_apply_macro_3d_component_masks( double* const*       dst,
                                                                                   const double* const* src,
                                                                                   const double*        mu,
                                                                                   const double*        macro_vertex_coords,
                                                                                   int64_t              micro_edges_per_macro_edge,
                                                                                   const unsigned*      masks /* 3 */,
                                                                                   int                  update,
                                                                                   hyteg_hip_stream_t   stream );
/* Fused form of P1ElementwiseOperator::smooth_jac (src/hyteg/elementwiseoperators/P1ElementwiseOperator.cpp:288-331) on the three
 * components, at the INNER points only:  dst_i = src_i + omega * inv_diag_i .* ( rhs_i - ( A src )_i ).  No dst may alias an input. */
HYTEG_HIP_API int hyteg_hip_p1_elementwise_epsilon_jacobi_macro_3d( double* const*       dst,
                                                                    const double* const* src,
                                                                    const double* const* rhs,
                                                                    const double* const* inv_diag,
                                                                    const double*        mu,
                                                                    const double*        macro_vertex_coords,
                                                                    int64_t              micro_edges_per_macro_edge,
                                                                    double               omega,
                                                                    hyteg_hip_stream_t   stream );
/* Fused residual of a multigrid cycle on the three components, at the INNER points only:  dst_i = rhs_i - ( A src )_i.  Replaces
 * the apply and the assign of GeometricMultigridSolver::solveRecursively (src/hyteg/solvers/GeometricMultigridSolver.hpp:240-246)
 * over three components: one pass over the arrays instead of seven.  comps: bit i set = component i is written (a component whose
 * bit is off is computed and not stored; 0 launches nothing).  No dst may alias an input, mu or another dst, and no input may be
 * mu (EINVAL).  Levels 0..8 (nothing to do below level 2). */
HYTEG_HIP_API int hyteg_hip_p1_elementwise_epsilon_residual_macro_3d( double* const*       dst,
                                                                      const double* const* src,
                                                                      const double* const* rhs,
                                                                      const double*        mu,
                                                                      const double*        macro_vertex_coords,
                                                                      int64_t              micro_edges_per_macro_edge,
                                                                      unsigned             comps,
                                                                      hyteg_hip_stream_t   stream );
/* The steps of ChebyshevSmoother::solve (src/hyteg/solvers/ChebyshevSmoother.hpp:165-212) on the three components, fused, at the
 * INNER points only, with the semantics of hyteg_hip_p1_chebyshev_start_cell / _step_cell above:
 *   start:  t_out_i = inv_diag_i .* ( rhs_i - ( A x )_i );  x is the stencil source and is not updated (x += c_0 t_out is deferred
 *           to the next step, or to a vector pass for a smoother of order 1)
 *   step:   t_out_i = inv_diag_i .* ( A t_in )_i,  x_i = ( x_i + c_prev t_in_i ) + c_cur t_out_i, the first summand only if
 *           has_prev != 0; x is read and rewritten at the output points only.
 * comps as above, for both store streams of the step.  A written array (t_out, x) must alias no other array of the call, and no
 * array may be mu (EINVAL).  Levels 0..8. */
HYTEG_HIP_API int hyteg_hip_p1_elementwise_epsilon_chebyshev_start_macro_3d( double* const*       t_out,
                                                                             const double* const* rhs,
                                                                             const double* const* x,
                                                                             const double* const* inv_diag,
                                                                             const double*        mu,
                                                                             const double*        macro_vertex_coords,
                                                                             int64_t              micro_edges_per_macro_edge,
                                                                             unsigned             comps,
                                                                             hyteg_hip_stream_t   stream );
HYTEG_HIP_API int hyteg_hip_p1_elementwise_epsilon_chebyshev_step_macro_3d( double* const*       t_out,
                                                                            double* const*       x,
                                                                            const double* const* t_in,
                                                                            const double* const* inv_diag,
                                                                            const double*        mu,
                                                                            const double*        macro_vertex_coords,
                                                                            int64_t              micro_edges_per_macro_edge,
                                                                            double               c_prev,
                                                                            double               c_cur,
                                                                            int                  has_prev,
                                                                            unsigned             comps,
                                                                            hyteg_hip_stream_t   stream );
/* Replaces computeInverseDiagonalOperatorValues of the three diagonal blocks (what P1EpsilonOperator.hpp's extractInverseDiagonal
 * reads): diag[i] += sum over the adjacent micro-cells e of this macro-cell of A_e^{ii}[a][a], at all points of the cell array. */
HYTEG_HIP_API int hyteg_hip_p1_elementwise_epsilon_diagonal_macro_3d( double* const*     diag,
                                                                      const double*      mu,
                                                                      const double*      macro_vertex_coords,
                                                                      int64_t            micro_edges_per_macro_edge,
                                                                      hyteg_hip_stream_t stream );
/* Tuning knobs as in b-4 (no counterpart in the reference): the brick shape of the inner-point z-march (0, 0 = the default of the
 * level; EINVAL for a shape that is not compiled in), and the inner points by the one-thread-per-point kernel instead.  The
 * Chebyshev step is not compiled at 2 x 4 (it would need scratch): with that shape set it marches ITS default shape of the level,
 * so a timing of the step taken under set_shape( 2, 4 ) is a timing of 1 x 4 (levels <= 7) or 1 x 8 (level 8). */
HYTEG_HIP_API int hyteg_hip_p1_elementwise_epsilon_set_shape( int ny, int lz );
HYTEG_HIP_API int hyteg_hip_p1_elementwise_epsilon_set_inner_by_points( int on );

/* ---- strong free-slip: projection onto the tangential plane ----------------------------------------------------------
 * Replaces vertexdof::macroface::projectNormal3D, vertexdof::macroedge::projectNormal3D and
 * vertexdof::macrovertex::projectNormal3D (src/hyteg/p1functionspace/freeslip/VertexDoFProjectNormal.hpp:43-97, 200-249,
 * 383-425) for all macro-cells of a chunk in ONE launch (grid.y = cell) at every level 0..11: at each shell point of cell c
 * whose macro-primitive slot bit is set in masks[c] (bit 14, the inner points, is ignored: they are never projected)
 *    d = n0 u + n1 v + n2 w;   u -= d n0,  v -= d n1,  w -= d n2        = ( I - n n^T ) ( u, v, w ), n NOT normalised.
 * u, v, w, normals: HOST arrays of `ncells` device pointers (1 <= ncells <= HYTEG_HIP_MAX_BATCH); normals[c] is the table
 * [3][hyteg_hip_p1_shell_size( level )] of cell c, component-major, indexed by the shell enumeration q below -- the reference
 * calls normal_function at every point of every call, here the caller evaluates it once.  No allocation, no upload, no
 * synchronisation: the call can be recorded into a graph. */
HYTEG_HIP_API int hyteg_hip_p1_project_normal_cells( int                  ncells,
                                                     double* const*       u,
                                                     double* const*       v,
                                                     double* const*       w,
                                                     const double* const* normals,
                                                     int                  level,
                                                     const unsigned*      masks,
                                                     hyteg_hip_stream_t   stream );
/* The shell enumeration of the kernels above and of hyteg_hip_p1_apply_cell_boundary, on the host: out[4 q + 0..3] =
 * x, y, z, slot of q in [0, hyteg_hip_p1_shell_size( level )); slot (0..13: edge0..5, face0..3, vertex0..3) is -1 for the q
 * the kernels skip (a point on a macro-edge or -vertex is visited through its lowest-numbered face only).  Replaces the
 * iterators vertexdof::macroface::Iterator( level, 1 ) / macroedge::Iterator( level, 1 ) of the loops cited above.
 * hyteg_hip_p1_shell_size: 4 tri( 2^level + 1 ), 0 for a level outside 0..11. */
HYTEG_HIP_API int hyteg_hip_p1_shell_size( int level );
HYTEG_HIP_API int hyteg_hip_p1_shell_enumeration( int level, int* out );

/* The same projection on the edge-DoF arrays of three P2 functions (replaces edgedof::macroface::projectNormal3D and
 * edgedof::macroedge::projectNormal3D, src/hyteg/edgedofspace/freeslip/EdgeDoFProjectNormal.hpp), levels 0..HYTEG_HIP_P2_MAX_LEVEL,
 * over the enumeration of the shell edge DoFs: per face of the cell the three orientations that lie in it, an edge DoF on a
 * macro-edge through its lowest-numbered face only -- every edge DoF of a macro-face or macro-edge slot once, no other.
 * normals[c]: [3][hyteg_hip_p2_edge_shell_size( level )], evaluated at the midpoints of the micro-edges; masks: bits 0..9.
 * hyteg_hip_p2_edge_shell_enumeration: out[5 q + 0..4] = x, y, z, orientation (0..5: X, Y, Z, XY, XZ, YZ), slot (-1: skipped);
 * hyteg_hip_p2_edge_shell_size: 12 tri( 2^level ), 0 for a level out of range.  They replace edgedof::macroface::Iterator /
 * edgedof::macroedge::Iterator of those loops. */
HYTEG_HIP_API int hyteg_hip_p2_edge_project_normal_cells( int                  ncells,
                                                          double* const*       u,
                                                          double* const*       v,
                                                          double* const*       w,
                                                          const double* const* normals,
                                                          int                  level,
                                                          const unsigned*      masks,
                                                          hyteg_hip_stream_t   stream );
HYTEG_HIP_API int hyteg_hip_p2_edge_shell_size( int level );
HYTEG_HIP_API int hyteg_hip_p2_edge_shell_enumeration( int level, int* out );

#ifdef __cplusplus
}
#endif
#endif /* HYTEG_HIP_H */
