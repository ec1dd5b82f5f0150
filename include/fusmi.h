/*
 * fusmi.h -- C ABI of libfusmi, the MI355X-native drop-in for the fenicsx-fus hot path:
 * sum-factorised mass/stiffness operator action on hex spectral elements + explicit RK4
 * stage update + shared-DOF halo exchange.  (SURVEY.md section 8b is the contract.)
 *
 * Each entry point names the reference interface it replaces (paths relative to the reference
 * repository adeebkor/fenicsx-fus @ 2024-10-08).  Plain pointers and sizes only; no C++ or
 * torch types cross this boundary.  All functions return FUS_OK (0) or a negative error code;
 * fus_last_error() returns the message of the calling thread's last failure.  Handles are not
 * thread-safe: one ctx/op/model per GPU per thread, like the reference's one object per MPI rank
 * (the reference operator holds mutable scratch, spectral_op.hpp:267-283).
 *
 * The library REQUIRES a HIP device: there is no CPU fallback.  Calls that need the device fail
 * with FUS_ERR_HIP when none is present.
 */
#ifndef FUSMI_H
#define FUSMI_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FUS_OK 0
#define FUS_ERR_ARG (-1)     /* invalid argument / unsupported P, tdim, dtype, geometry order */
#define FUS_ERR_HIP (-2)     /* HIP runtime error (including: no device) */
#define FUS_ERR_RCCL (-3)    /* RCCL error */
#define FUS_ERR_STATE (-4)   /* call sequence error (e.g. model used before init) */
#define FUS_ERR_LIMIT (-5)   /* a block does not fit the 160 KB LDS budget / index overflow */

enum { FUS_F32 = 0, FUS_F64 = 1 };           /* scalar type T of the reference templates */
enum { FUS_HOST = 0, FUS_DEVICE = 1 };       /* memory space of caller vectors */
enum { FUS_LINEAR = 0, FUS_LOSSY = 1, FUS_WESTERVELT = 2 };
enum { FUS_U = 0, FUS_V = 1 };

typedef struct fus_ctx fus_ctx;
typedef struct fus_op fus_op;
typedef struct fus_model fus_model;

const char* fus_last_error(void);
/* ABI version, for the binding to check. */
int fus_version(void);

/* ---- context --------------------------------------------------------------------------------
 * Replaces the implicit per-rank process state of the reference (MPI_COMM_WORLD rank,
 * Linear.hpp:64-65).  Binds to HIP device `device`, creates the compute and comm streams. */
int fus_init(int device, fus_ctx** ctx);
int fus_finalize(fus_ctx* ctx);
int fus_synchronize(fus_ctx* ctx);
/* Tunables, set before fus_op_create: "block_elems" (elements per LDS block) and "waves"
 * (waves per workgroup, 1..8): default 0 = auto (hexahedra with G streamed: 128 / 64 / 32 /
 * 20 / 12 / 8 elements at P = 2..7 in fp64, 128 / 64 / 48 / 24 / 24 / 16 in fp32, about half of
 * that -- 8 at P >= 5 -- on the affine and trilinear paths; 4 waves), "geometry" (0 auto: 7 numbers
 * per cell when every cell is a parallelepiped, else -- first-order hexahedra -- the 21 coefficients
 * of each cell's trilinear map with J and G recomputed per point in the kernel, else the streamed
 * per-point factors | 1 always stream the per-point factors, the reference's data path | 2 as auto
 * without the affine shortcut), "fields" (1 | 2: operator inputs the block kernel
 * stages per pass; 2 is required by FUS_LOSSY), "deterministic" (1: elements accumulate in
 * conflict-free rounds, results bitwise reproducible; 0 (default): LDS floating-point atomics, the
 * order of the <= 8 adds per DOF inside a block is free).
 * "forms" (set before fus_model_create; FUS_LOSSY / FUS_WESTERVELT): 0 (default) the C++ benchmark
 * forms -- absorbing and delta-mass terms on every listed boundary facet (BM7-SC1/forms.py:37-42),
 * source doubled (Lossy.hpp:216-220); 1 the Python package's -- those terms on tag 2 only, source
 * not doubled (python/src/fenicsxfus/_lossy.py:107-128, :186-189).
 * "external_transport" (1, before fus_comm_init: the caller exchanges the interface values, see below).
 * Multi-rank, set before fus_comm_init / fus_model_create: "overlap_blocks" (1: the blocks touching
 * interface DOFs are launched first and the exchange overlaps the remaining blocks; default 0: it
 * overlaps the shared-DOF kernel only), "halo_loopback" (1: timing rehearsal on one GPU -- a 1-rank
 * communicator, every send/receive goes to the own rank; results are not the physical ones).
 * "graph" (1: on one rank the launches of an RK step are captured and replayed as one hipGraph, the
 * executable graph being updated in place with each step's stage scalars; for launch-bound sizes
 * such as BASELINE config 1; default 0).
 * "lean_rk4" (set before fus_model_create; default 1): the classical RK4 keeps no accumulators u_, v_ of
 * Linear.hpp:282-294 in HBM -- the stage slopes are affine in the stage velocities, so the last stage builds the
 * new state from the three stage velocities (three rotating buffers), and u0 is rebuilt from the stage input the
 * kernel already holds in LDS (208 instead of 296 bytes of vector traffic per DOF and step, same arithmetic up
 * to rounding); 0 keeps them in HBM at every stage.  The Runge-Kutta orders 1-3 always keep them.
 * "mfma" (-1 auto (default) | 0 | 1, before fus_op_create): degrees 6 and 7 on the per-cell geometry
 * paths -- the index-1 / index-2 contractions of an element, the (N x N).(N x N^2) products of the
 * reference's contract<> (sum_factorisation.hpp:70-86), as 16x16x4 MFMA tiles on the matrix cores
 * instead of vector FMAs.  Auto = where it measures faster on MI355X: nowhere at present (the re-mapped vector form is
 * 3 % ahead of it at degree 7, fp64, trilinear geometry, the one case it used to win; profiles/r02_experiments.md).
 * "pack32" (-1 auto (default) | 0 | 1, before fus_op_create): fp32, degrees 5-7, per-cell geometry paths -- a
 * wave works on two elements at once, every tile exchange and FMA packed as float2 (half the LDS and vector
 * instructions per element of the scalar fp32 kernel, which is LDS bound).
 * "walk" (0 (default) | 1..8 | -1, any time): block-kernel workgroups per CU that walk several blocks each
 * with the next block's prologue loads in flight under the current block's epilogue; 0 = one workgroup
 * per block (measured faster everywhere so far, profiles/r02_experiments.md), -1 = as many as are resident.
 * "diag_metric" (1 (default) | 0, before fus_op_create): affine meshes whose cells have mutually orthogonal edges
 * take the diagonal-metric form of the stiffness kernel (fus_op_uses_diag_metric); 0 keeps the general affine form.
 * "planes" (1 (default) | 0 | 2..16, any time): the shared-dof stage kernel reads the block partial sums of a dof as
 * planes at the dof's own index (no index list; every access coalesced) or through the shared-dof CSR; the
 * sums and their order are the same.  The CSR form is also taken when a dof has more sharing blocks than the
 * kernel has planes (16; a value k = 2..16 lowers that limit to k).
 * "rayleigh_chunks" (0 (default) | 1..1024, any time): the number of source chunks fus_rayleigh splits its sum into; 0 = as
 * many as fill the device (see "transducers").
 * Unknown keys -> FUS_ERR_ARG. */
int fus_set_option(fus_ctx* ctx, const char* key, int64_t value);

/* Multi-GPU: one process per GPU.  fus_comm_unique_id fills a 128-byte RCCL id on rank 0; the
 * caller broadcasts it (any transport) and every rank calls fus_comm_init.  Replaces
 * MPI_Init/MPI_COMM_WORLD inside PetscInitialize (BM7-SC1/main.cpp:22). */
int fus_comm_unique_id(void* id128);
int fus_comm_init(fus_ctx* ctx, int rank, int nranks, const void* id128);
/* Diagnostic: n doubles through grouped ncclSend/ncclRecv to the own rank on the library stream
 * (checks the run-time RCCL binding; RCCL is dlopen'ed, preferring a copy already resident in the
 * process such as PyTorch's, or $FUSMI_RCCL). */
int fus_comm_selftest(fus_ctx* ctx, int64_t n);
/* In-place all-reduce of n host doubles over the ranks of fus_comm_init (RCCL): the global minimum
 * cell size behind the time step (MPI_Reduce(MIN) + MPI_Bcast,
 * cpp/fenicsx-sf-naive/examples/linear_planewave2d_1/main.cpp:67-68) and the sums behind norms
 * (:151-157).  One rank: no-op.  In-process groups / external transport: FUS_ERR_STATE (the caller
 * holds every rank's value, or its own transport). */
#define FUS_SUM 0
#define FUS_MIN 1
#define FUS_MAX 2
int fus_comm_allreduce(fus_ctx* ctx, double* values, int n, int op);

/* In-process transport for rehearsing the multi-rank path on ONE GPU (tests): the n contexts of
 * this process become ranks 0..n-1 and interface planes move by device copies instead of RCCL.
 * Models of such contexts are finished with fus_group_finish_setup (the sharers' parts of m and
 * of the boundary weights) and advanced in lock-step with fus_group_rk4_steps.  One stage loop steps every member,
 * so the members of a group agree in rk_order, model kind and scalar type: otherwise FUS_ERR_ARG before any launch. */
int fus_comm_init_local(fus_ctx** ctxs, int n);

/* ---- operator data ------------------------------------------------------------------------
 * Replaces the constructors StiffnessSpectral3D<T,P>(V) / MassSpectral3D<T,P>(V)
 * (cpp/fenicsx-sf/common/spectral_op.hpp:135-171, :32-63): takes the tensor-ordered cell dofmap
 * (what reorder_dofmap, permute.hpp:15-42, produces), the 1-D node coordinates on [0,1] in the
 * caller's local order (any order; the library derives GLL weights and the derivative table
 * for it, replacing tabulate_1d precompute.hpp:217-234) and the mesh geometry, and computes on
 * the device the scaled geometric factors G = J^-1 J^-T |detJ| w and |detJ| w
 * (compute_scaled_geometrical_factor / _jacobian_determinant, precompute.hpp:101-213, 33-94).
 * One object serves both operators (the reference builds one per operator, Lossy.hpp:152-153).
 *   tdim        3 (hexahedra) or 2 (quadrilaterals: StiffnessSpectral2D / MassSpectral2D,
 *               cpp/fenicsx-sf-naive/common/spectral_op.hpp:29-107, 226-359; N^2 nodes per cell,
 *               geom_dofmap int32[ncells * 4] with v = vx + 2vy (order 1) or int32[ncells * 9] with
 *               n = nx + 3ny (order 2, biquadratic), G has 3 entries (xx, xy, yy) per point, local
 *               facets 0..3 = y=0, x=0, x=1, y=1)
 *   P           polynomial degree 2..10 (the reference's Qdegree map, spectral_op.hpp:35-44); N = P+1 nodes per
 *               direction.  Degrees 8-10: first-order hexahedra through the per-cell geometry paths only
 *               ("geometry" 0 or 2); a tensor plane then has more than 64 columns and two waves share an element
 *   dtype       FUS_F64 | FUS_F32: type of geom_x and of every vector/coefficient argument later
 *   tensor_dofmap  int32[ncells * N^tdim], local DOF indices < ndofs, x-slowest tensor order
 *   nodes1d     double[N]
 *   geom_x      T[nnodes * 3]
 *   geom_order  1: geom_dofmap int32[ncells * 8], vertex order v = vx + 2vy + 4vz (DOLFINx's);
 *               2: geom_dofmap int32[ncells * 27], nodes in tensor order n = nx + 3ny + 9nz with
 *                  n_d in {0,1,2} <-> reference coordinate {0, 1/2, 1} (the caller permutes from
 *                  DOLFINx's vertices-edges-faces-interior order).  Other orders -> FUS_ERR_ARG.
 * All arrays are caller-owned host memory, copied during the call. */
int fus_op_create(fus_ctx* ctx, int tdim, int P, int dtype, int64_t ncells, int64_t ndofs,
                  const int32_t* tensor_dofmap, const double* nodes1d, const void* geom_x,
                  int64_t nnodes, const int32_t* geom_dofmap, int geom_order, fus_op** op);
int fus_op_destroy(fus_op* op);

/* y += K(coeffs) x.  Replaces StiffnessSpectral3D::operator()(x, coeffs, y)
 * (spectral_op.hpp:173-243): y is ACCUMULATED, x must hold every local DOF value (the caller's
 * scatter_fwd, Linear.hpp:196), coeffs has one scalar per local cell.  No inter-rank reduction is
 * done (the caller's scatter_rev, Linear.hpp:206).  x, coeffs, y: T arrays in `space`. */
int fus_stiffness_apply(fus_op* op, const void* x, const void* coeffs, void* y, int space);
/* y += M(coeffs) x.  Replaces MassSpectral3D::operator() (spectral_op.hpp:69-86). */
int fus_mass_apply(fus_op* op, const void* x, const void* coeffs, void* y, int space);

/* Inspection (parity tests): geometry factors in the REFERENCE layout G[cell][point][6]
 * (xx,xy,xz,yy,yz,zz), detJ[cell][point] (precompute.hpp:198-208); host T arrays, may be NULL. */
int fus_op_get_geometry(fus_op* op, void* G, void* detJ);
/* 1-D tables in the caller's node order: weights[N], dphi[N*N] row = point (spectral_op.hpp:168). */
int fus_op_get_tables(fus_op* op, double* weights, double* dphi);
/* Layout statistics: out[0]=nblocks out[1]=interior dofs out[2]=shared dofs out[3]=(block,dof)
 * pairs out[4]=max local dofs per block out[5]=unique block shapes out[6]=LDS bytes per block
 * out[7]=padded internal vector length. */
int fus_op_info(fus_op* op, int64_t out[8]);
/* 1 when every cell was found to be a parallelepiped and the operator rebuilds G = Gc w_q from 7
 * numbers per cell instead of streaming 6 per point (option "geometry" = 0, the default); 0
 * otherwise (see fus_op_geometry_mode). */
int fus_op_is_affine(fus_op* op);
/* Geometry source of the block operator: 0 = per-point factors streamed from HBM (the reference's
 * data path, precompute.hpp:101-213), 1 = affine cells (7 numbers per cell), 2 = first-order
 * hexahedra with the Jacobian recomputed per point from the cell's trilinear map (21 numbers per
 * cell; the default for first-order meshes with non-affine cells). */
int fus_op_geometry_mode(fus_op* op);
/* 1 when the operator's block kernel runs its index-1 / index-2 contractions on the matrix cores
 * (MFMA 16x16x4; degrees 6 and 7 on the per-cell geometry paths, option "mfma"). */
int fus_op_uses_mfma(fus_op* op);
/* 1 when the affine kernel runs in its diagonal-metric form: every cell a parallelepiped with mutually orthogonal
 * edges (boxes in any orientation; J^T J and with it G of spectral_op.hpp:113-130 are diagonal), degrees <= 7 --
 * the stiffness action as three 1-D stiffness contractions, sum_d g_d (M x K1 x M) x with K1 = D^T diag(w) D,
 * instead of the six derivative contractions and the pointwise transform (option "diag_metric"). */
int fus_op_uses_diag_metric(fus_op* op);
/* 1 when the block kernel runs its index-1 contraction on v_mfma_f64_4x4x4_4b_f64 straight from the registers (degree 7,
 * fp64, first-order hexahedra with non-affine cells -- the trilinear geometry kernel; the default there): the reference's
 * contract<T,8,8,8,8,bool> of spectral_op.hpp:199-201 / :222-227 (sum_factorisation.hpp:70-86) on the matrix cores. */
int fus_op_uses_mfma4(fus_op* op);
/* 1 when the fp32 stiffness kernel works on two elements per wave in packed float2 (degrees 5-7, per-cell
 * geometry paths, LDS-atomic accumulation; option "pack32"). */
int fus_op_uses_pack32(fus_op* op);
/* 1 when a launch of the operator with one workgroup per block runs the block kernel that keeps its block loop and
 * every leftover loop: streamed geometry, or a layout with a block larger than the unrolled first batches of the
 * straight-line kernel (fp64, per-cell geometry, degrees <= 4; lower block_elems to get that kernel back).  Answered
 * for launches with as many inputs as the operator was created for (option "fields"): an operator created for two
 * inputs also runs one-input launches (the mass action, the plain stiffness action), whose batches are larger and may
 * fit where the two-input ones do not.  Option "walk" != 0 selects the same kernel per launch, wherever a launch has
 * fewer workgroups than blocks; that choice depends on the launch's number of blocks and is not reported here. */
int fus_op_uses_block_loop(fus_op* op);
/* Smallest cell size of the local mesh, the size of a cell being its largest vertex-to-vertex
 * distance (dolfinx::mesh::h, linear_planewave2d_1/main.cpp:60-64); dt = CFL hmin / (c P^2), :102. */
int fus_op_hmin(fus_op* op, double* hmin);
/* out = sum over the local cells of the GLL-quadrature integral of x^2 (caller numbering; loc =
 * FUS_HOST | FUS_DEVICE); the sum over ranks is the squared L2 norm of
 * fem::assemble_scalar(u*u*dx), linear_planewave2d_1/main.cpp:151-157. */
int fus_op_norm2(fus_op* op, const void* x, int loc, double* out);

/* out[dof] += cellcoef[cell] * |J_facet| w_a w_b at the GLL nodes of each listed boundary facet,
 * facets given as (cell, local facet) pairs in DOLFINx numbering (hex: 0:z=0 1:y=0 2:x=0 3:x=1
 * 4:y=1 5:z=1), the pairs fem::compute_integration_domains returns (Linear.hpp:113-118).
 * Replaces the FFCx facet kernels of the GLL-collocated forms L/a (SC1-BM1/forms.py:36-39,
 * BM7-SC1/forms.py:37-42), which are diagonal.  Host arrays; out is T[ndofs]. */
int fus_facet_diag(fus_op* op, int64_t nfacets, const int32_t* facet_cells,
                   const int32_t* facet_local, const void* cellcoef, void* out);

/* Shared-DOF description for >1 rank (replaces the IndexMap ghost/owner data behind
 * la::Vector::scatter_fwd/scatter_rev, Linear.hpp:196-206): for neighbour k, the local DOF
 * indices shared with rank ranks[k], counts[k] of them, concatenated in dof_idx; both sides
 * must list a shared set in the same (global id) order.  Call once, right after fus_op_create and
 * before any model is created on the op (the block layout is rebuilt so that these DOFs are never
 * finished inside a block's fused epilogue). */
int fus_op_set_neighbours(fus_op* op, int nneigh, const int32_t* ranks, const int64_t* counts,
                          const int32_t* dof_idx);

/* ---- model ------------------------------------------------------------------------------------
 * Replaces LinearSpectral3D<T,P>(element, mesh, facet_tags, c0, rho0, freq, amp, speed)
 * (Linear.hpp:55-158): c0, rho0 are the DG0 arrays (T[ncells]); boundary facets as
 * (cell, local facet, tag) with tag 1 = source, 2 = absorbing (forms.py:38-39).  Builds the lumped
 * mass m (Linear.hpp:127-134) and the operator coefficient -1/rho (:154-155) on the device.
 * FUS_LOSSY replaces LossySpectral3D (Lossy.hpp:56-173): delta0 = diffusivity of sound per cell; the
 * two operator actions of a stage, lin_op(u_n, -1/rho) and att_op(v_n, -delta/(rho c^2))
 * (Lossy.hpp:231-232), run as ONE pass of the block kernel (both share G); absorbing term on every
 * listed facet, dg source term and the delta/(rho c^3) boundary mass term as in
 * BM7-SC1/forms.py:37-42; source scaling 2 W p0 w0/s0 as live in Lossy.hpp:216-220.  The operator
 * data must have been created with option "fields" = 2.
 * FUS_WESTERVELT replaces WesterveltSpectral3D (Westervelt.hpp:58-193): beta0 = coefficient of
 * nonlinearity per cell.  The per-stage mass re-assembly m = m0 + M(nlin1) u_n and the RHS term
 * M(nlin2)(v_n^2) (Westervelt.hpp:246-265) are diagonal (M(c) x = diag(M(c) 1) .* x), so they fold
 * into the fused stage update: kv = (b - mn1 v_n^2) / (m0 + mn1 u_n), mn1 = M(-2 beta/(rho^2 c^4)) 1. */
int fus_model_create(fus_ctx* ctx, int kind, fus_op* op, const void* c0, const void* rho0,
                     const void* delta0, const void* beta0, int64_t nfacets,
                     const int32_t* facet_cells, const int32_t* facet_local,
                     const int32_t* facet_tags, double freq, double amp, double speed,
                     fus_model** model);
int fus_model_destroy(fus_model* model);
/* Explicit Runge-Kutta scheme of the Python reference (python/src/fenicsxfus/_linear.py:286-311):
 * 1 forward Euler, 2 / 3 Ralston, 4 classical (default; the only one the C++ reference has,
 * Linear.hpp:263-265).  The entry points named rk4 run the selected scheme. */
int fus_model_set_rk_order(fus_model* model, int order);
/* u_n = v_n = 0 (Linear.hpp:161-164). */
int fus_model_init(fus_model* model);
/* Classical RK4 from t0 to tf with step dt, `while (t < tf) { dt = min(dt, tf - t); ... }`
 * (Linear.hpp:228-314); *nsteps receives the number of steps taken (may be NULL). */
int fus_model_rk4(fus_model* model, double t0, double tf, double dt, int64_t* nsteps);
/* Exactly nsteps full steps of size dt starting at t0 (benchmark entry; same stage arithmetic). */
int fus_model_rk4_steps(fus_model* model, double t0, double dt, int64_t nsteps);
/* Copy u_n (FUS_U) or v_n (FUS_V) out / in, caller DOF numbering, T[ndofs] in `space`
 * (u_sol(), Linear.hpp:316). */
int fus_model_get(fus_model* model, int which, void* out, int space);
int fus_model_set(fus_model* model, int which, const void* in, int space);
/* Lumped mass vector m in caller numbering (host T[ndofs]); parity inspection. */
int fus_model_get_mass(fus_model* model, void* out);
int64_t fus_model_ndofs(fus_model* model); /* number_of_dofs(), Linear.hpp:318 (local) */

/* ---- receivers: point samples of the resident solution ------------------------------------------
 * Replaces Function::eval(points, cells) after the cell search of compute_eval_params
 * (python/src/fenicsxfus/utils.py:10-47) / geometry::compute_colliding_cells
 * (cpp/mwe/parallel_eval_line/main.cpp:49-84): the caller locates each point (cell = local cell index in caller
 * numbering, refcoords = its reference coordinates in [0,1]^tdim, double[npts*tdim], X0 pairing with tensor index
 * 0 of the dofmap) and drops points outside the local mesh, as the reference does (points_on_proc).  The library
 * keeps, per receiver, the internal indices of its cell's dofs and the 1-D Lagrange basis values, and evaluates
 * u_h (FUS_U) or v_h (FUS_V) at the receivers from the vectors resident in HBM -- no full-vector copy.
 *   fus_model_sample       T[npts] now, into host or device memory (`space`)
 *   fus_model_record       sample `which` after every `every`-th step into a device buffer of `capacity` records
 *                          (every = 0: off); restarts the record count; `capacity` is the limit of this recording,
 *                          whatever an earlier call asked for.  A step is one of fus_model_rk4 /
 *                          fus_model_rk4_steps, of fus_group_rk4_steps (every member records by itself) or, under the
 *                          external transport, the fus_model_stage_end of a step's last stage (time t + dt).  A rank
 *                          that holds none of the receivers (npts = 0) counts its records and their times all the same
 *   fus_model_get_records  copies the records taken so far (T[nrec*npts], row = record) and their times; out / times
 *                          may be NULL to query *nrec only */
int fus_model_set_receivers(fus_model* model, int64_t npts, const int32_t* cells, const double* refcoords);
int fus_model_sample(fus_model* model, int which, void* out, int space);
int fus_model_record(fus_model* model, int which, int every, int64_t capacity);
int fus_model_get_records(fus_model* model, void* out, double* times, int64_t* nrec);

/* ---- field monitor: whole-field maps over the last source periods, accumulated on the device ---------
 * What a focused-ultrasound user reads from a run -- peak positive / peak negative pressure, RMS pressure, amplitude
 * and phase of the fundamental and its harmonics (the reference validates its Westervelt runs against the Fubini
 * series, python/tests/test_westerveltspectral_1d.py:85-111) -- without a full-vector copy per step: after selected
 * steps one kernel folds the resident state into per-DOF accumulators in HBM (the receivers' pattern, from points
 * to the whole field).
 *
 * Sampling.  Let s be the number of steps completed since fus_model_monitor was called.  After step s a sample j is
 * taken when   s > skip   and   (s - skip) % every == 0   and   (count == 0 or fewer than count samples so far).
 * The sampled vector x_j is the one fus_model_get returns for `which` (FUS_U | FUS_V) at that moment; the sample
 * time t_j is the step's end time as the time loop holds it (the value the receivers' records carry; in
 * fus_model_rk4 with FUS_F32 the float time, in fus_model_stage_end t + dt).  Steps are counted in fus_model_rk4,
 * fus_model_rk4_steps, fus_group_rk4_steps (every member) and in fus_model_stage_end of the last stage.
 * Accumulators, per DOF of the internal vector (n_internal of them, fus_op_info out[7]):
 *   running max  max_j x_j, running min  min_j x_j                                    type T
 *   sum  S = sum_j x_j,  sum of squares  Q = sum_j x_j^2                              double
 *   C_k = sum_j x_j cos(2 pi k f t_j),  S_k = sum_j x_j sin(2 pi k f t_j), k = 1..nharm    double
 * The sums are double also for FUS_F32 models.  The 2 nharm phase factors of a sample are computed on the host in
 * double and passed to the kernel by value; the kernel calls no trigonometric function.
 * Returned quantities, n = number of samples:
 *   FUS_MON_MAX  running max          FUS_MON_MIN  running min
 *   FUS_MON_MEAN S / n                FUS_MON_RMS  sqrt(Q / n)
 *   FUS_MON_COS  (2 / n) C_k          FUS_MON_SIN  (2 / n) S_k
 * Over a window of whole periods with uniform sampling, x ~ MEAN + sum_k COS_k cos(2 pi k f t) + SIN_k sin(2 pi k f t).
 * Aliasing: the samples per period, 1 / (f dt every), must exceed 2 nharm.
 * Memory: n_internal * (2 sizeof(T) + (2 + 2 nharm) * 8) bytes of accumulators; a sample reads the state once and
 * reads and writes every accumulator once.
 *   fus_model_monitor       nharm in 0..8; freq == 0: the model's source frequency; every == 0 switches the monitor
 *                           off and frees the accumulators; any other call allocates and zeroes them and restarts
 *                           s and n (FUS_ERR_HIP naming the bytes asked for when the allocation fails; a failed
 *                           restart leaves the monitor off, the earlier accumulators are gone)
 *   fus_model_monitor_get   quantity = FUS_MON_*, k in 1..nharm for FUS_MON_COS / FUS_MON_SIN (ignored otherwise);
 *                           out = T[ndofs] in caller numbering, host or device memory (`space`).  FUS_ERR_STATE
 *                           while n == 0 or the monitor is off.  The accumulators are not altered: sampling may
 *                           continue afterwards
 *   fus_model_monitor_info  number of samples so far, times of the first and the last one (each may be NULL; the
 *                           times are 0 while n == 0).  FUS_ERR_STATE while the monitor is off */
enum { FUS_MON_MAX = 0, FUS_MON_MIN = 1, FUS_MON_MEAN = 2, FUS_MON_RMS = 3, FUS_MON_COS = 4, FUS_MON_SIN = 5 };
int fus_model_monitor(fus_model* model, int which, int nharm, double freq, int64_t skip, int every, int64_t count);
int fus_model_monitor_get(fus_model* model, int quantity, int k, void* out, int space);
int fus_model_monitor_info(fus_model* model, int64_t* nsamples, double* t_first, double* t_last);

/* ---- gradient: the sum-factorised gradient of a nodal field, recovered at the DOFs ---------------------------------
 * Every other quantity the library reports is a function of a field at a point; these two calls differentiate one.
 * Per element e the kernel gathers the field, takes the reference derivatives with the derivative table the stiffness
 * action starts with (spectral_op.hpp:194-210), and at every GLL node q forms J(q), K = J^-1 and
 *   (grad x)_e(q) = K(q)^T grad_xi x_e(q),        W_e(q) = |det J_e(q)| w_q   (the mass operator's factor),
 * J from the cell's coordinates (trilinear / triquadratic, 2-D bilinear / biquadratic map), whatever geometry mode the
 * operator runs in: no per-point geometry array is needed.  With (e,q)->i meaning that node q of element e is DOF i:
 *   gradient:  y_d[i] += sum_{(e,q)->i} c_e W_e(q) (grad x)_{e,d}(q)
 *   pairs:     y_d[i] += sum_{(e,q)->i} W_e(q) sum_{k<K} c_{k,e} [ a_k(i) (grad b_k)_{e,d}(q) - b_k(i) (grad a_k)_{e,d}(q) ]
 * The recovered nodal value is the lumped-mass L2 projection g_d[i] = y_d[i] / sum_{(e,q)->i} W_e(q); the denominator is
 * M(1) 1, computed once per operator with the mass action and kept.
 * Arithmetic: the element work is done in T, the sums over the elements of a DOF in double for both scalar types and
 * rounded to T once per block; the partial sums of a DOF that several blocks hold are added in T in ascending block order.
 * The elements of a block are visited in the layout's conflict-free rounds, so the result is the same bits on every call,
 * with or without the context option "deterministic".
 * Every operator fus_op_create accepts is covered (degrees 2-10, both scalar types, both cell types and geometry orders,
 * any block size); a block whose image does not fit LDS with all components runs one launch per component.
 * fus_op_gradient_plan reports what a call on this operator launches: out[0] = kernel launches per call (1, or tdim
 * component passes), out[1] = components per launch, out[2] = threads per element group, out[3] = LDS bytes per workgroup.
 *   out     T[tdim][ndofs], component-major, caller numbering, `space`
 *   mode    FUS_GRAD_WEIGHTED: out is ACCUMULATED with the weighted sums y_d -- no inter-rank reduction, the
 *           fus_stiffness_apply convention: a caller with its own transport sums them over the sharers of a DOF and divides
 *           by the equally summed fus_mass_apply(1, 1).
 *           FUS_GRAD_NODAL: out is OVERWRITTEN with g_d (local denominators: complete on one rank)
 *   coeffs  fus_op_gradient: T[ncells] or NULL (= 1); fus_op_gradient_pairs: T[npairs][ncells]
 *   a, b    T[npairs][ndofs], caller numbering; npairs in 1..8
 * FUS_ERR_ARG: a null pointer, npairs outside 1..8, a mode or space that does not exist. */
enum { FUS_GRAD_WEIGHTED = 0, FUS_GRAD_NODAL = 1 };
int fus_op_gradient(fus_op* op, const void* x, const void* coeffs, void* out, int mode, int space);
int fus_op_gradient_pairs(fus_op* op, int npairs, const void* a, const void* b, const void* coeffs,
                          void* out, int mode, int space);
int fus_op_gradient_plan(fus_op* op, int64_t out[4]);

/* ---- intensity: time-averaged intensity vector and radiation force from the monitor's harmonic maps -----------------
 * For p_k(t) = C_k cos(w_k t) + S_k sin(w_k t) (C_k = FUS_MON_COS, S_k = FUS_MON_SIN, w_k = 2 pi k f) and the first-order
 * momentum equation rho dw/dt = -grad p, the time-averaged intensity I = <p w> is
 *   I = sum_k (C_k grad S_k - S_k grad C_k) / (2 rho w_k)          (p = A cos(w t - kappa x): A^2 / (2 rho c) along +x),
 * the pair form above with a_k = C_k, b_k = S_k.  fus_model_intensity evaluates
 *   out = nodal  sum_{k=1..nharm} coef[k-1][e] (C_k grad S_k - S_k grad C_k)
 * on the device from the model's monitor accumulators: the kernel reads the double planes in place, scales them by 2 / n
 * and rounds them to T exactly as fus_model_monitor_get does, then works in T -- the result is the pair form applied to
 * the maps the caller could have pulled.
 *   coef    NULL: 1 / (2 rho_e w_k) with the monitor's frequency f -- the intensity in W/m^2; else T[nharm][ncells] in
 *           `space` (e.g. alpha_k / (rho c w_k): the radiation force density F = sum_k 2 alpha_k I_k / c in N/m^3)
 *   out     T[tdim][ndofs], component-major, caller numbering, `space`
 * The call alters neither the wave state nor any monitor accumulator: sampling may continue afterwards.
 * FUS_ERR_ARG: a null model or out, nharm outside 1..8, a non-finite coef.  FUS_ERR_STATE: the monitor is off, watches
 * FUS_V or has taken no sample yet (looked at before nharm's range, so a caller that asks for "all the monitor holds"
 * with the monitor off gets this answer); it holds fewer harmonics than nharm; the model's operator has neighbours: the sums
 * over the sharers of an interface DOF have no exchange here (fus_op_gradient_pairs with FUS_GRAD_WEIGHTED on pulled maps
 * is the building block for a caller with its own transport).
 * Lossy, Westervelt and relaxation models: rho dw/dt = -grad p is the first-order momentum equation; the viscous and
 * nonlinear corrections to the particle velocity w are not modelled. */
int fus_model_intensity(fus_model* model, int nharm, const void* coef, void* out, int space);

/* ---- phased and apodised sources: per-DOF amplitude, delay and tone burst -----------------------------------------
 * The reference's source is one scalar g(t) times the diagonal facet weights of the tag-1 boundary (Linear.hpp:185-192,
 * :204-205), so every DOF of that boundary radiates with the same amplitude and phase.  This call gives each DOF d of it
 * an amplitude factor a_d >= 0 and a delay tau_d >= 0 -- electronic focusing and steering of a flat aperture, as array
 * transducers do it -- and optionally makes the source a tone burst.
 *
 * Waveform.  With the local time s = t - tau_d, the source frequency f, w0 = 2 pi f, the ramp length Lr = 4 / f (the
 * reference's window_length), the duration D (0 = continuous) and C = scale p0 w0 / s0 (scale = 2 for FUS_LOSSY /
 * FUS_WESTERVELT with option "forms" = 0, else 1, as for the default source):
 *   W(s)  = 0                                  for s <= 0, and for s >= D when D > 0
 *         = (1 - cos(pi f s / 4)) / 2          for 0 < s < Lr
 *         = (1 - cos(pi f (D - s) / 4)) / 2    for D - Lr < s < D when D > 0
 *         = 1                                  otherwise
 *   g_d(t)  = a_d C W(s) cos(w0 s)
 *   dg_d(t) = a_d C (W'(s) cos(w0 s) - W(s) w0 sin(w0 s))       (the dg term of FUS_LOSSY / FUS_WESTERVELT)
 * The source of a DOF is exactly 0 for t <= tau_d (and for t >= tau_d + D), so nothing radiates before its delay has
 * passed.  With a = 1, tau = 0, D = 0 and t >= 0 this is the default source.  Evaluated in double for both scalar types
 * at the stage time the default source uses, rounded to T with the facet weight.
 *   amplitude, delay   T[ndofs] in caller numbering, host or device memory (`space`); NULL = 1 everywhere / 0 everywhere.
 *                      Values at DOFs off the source boundary are ignored; a negative or non-finite value at a DOF on
 *                      it -> FUS_ERR_ARG, the source stays as it was
 *   duration           D: 0 or >= 2 Lr = 8 / f; 0 < D < 2 Lr (the ramps would overlap) -> FUS_ERR_ARG
 * amplitude == NULL, delay == NULL, duration == 0 restores the default source and frees the arrays.  Amplitude only
 * (delay == NULL, duration == 0): the amplitude is folded into the facet weights once and a step enqueues what it
 * always did.  Otherwise one small kernel launch per new stage time (classical RK4: two per step, its two middle
 * stages share a time and its last one the next step's first) writes weight x g_d(stage time) for the boundary
 * entries -- profile name "source" -- and the stage kernels run unchanged.
 * Legal once the model's setup is finished (FUS_ERR_STATE before) and between steps; the state is kept.  Several ranks:
 * every sharer of a DOF passes the same values for it (they are functions of position). */
int fus_model_set_source(fus_model* model, const void* amplitude, const void* delay, double duration, int space);

/* ---- transducers: the Rayleigh integral of a radiating surface outside the mesh ------------------------------------
 * A bowl or an array radiates into a homogeneous coupling medium (sound speed c, density rho, absorption alpha in Np/m;
 * 0 for water) before its field reaches the meshed region.  With the time convention p(x,t) = Re[P(x) e^{-i w t}] --
 * P = COS_1 + i SIN_1 in the monitor's terms -- and surface points x_s of complex volume velocity q_s = v_n(x_s) dA_s in
 * m^3/s, w = 2 pi f, k = w / c, r_s = |x - x_s|:
 *   P(x)      = -(i w rho / 2 pi) sum_s q_s e^{i k r_s} e^{-alpha r_s} / r_s
 *   grad P(x) = -(i w rho / 2 pi) sum_s q_s (i k - alpha - 1/r_s) e^{i k r_s} e^{-alpha r_s} / r_s  (x - x_s) / r_s
 * A pair with r_s == 0 contributes nothing; rmin then reports 0, so the caller can see it.  3-D only.
 * fus_rayleigh evaluates this at ntgt targets.  It touches no operator or model; on several ranks each rank calls it
 * for its own DOFs and nothing is exchanged.  Evaluated on the source face of a box and turned into per-DOF amplitude
 * and delay (fenicsxfus_amd.transducer.drive) it is the boundary drive of fus_model_set_source: in steady state the
 * tag-1 term is facet weight x g_d(t), g_d = a_d C cos(w (t - tau_d)) the outward normal derivative of p, so
 * G = dP/dn_out where the source facets carry no absorbing term (FUS_LINEAR; Lossy / Westervelt with "forms" = 1) and
 * G = dP/dn_out - (i w / c) P where they do ("forms" = 0), a_d = |G_d| / C, tau_d = arg(G_d) / w wrapped into [0, 1/f).
 *
 * Arithmetic, per (target, source) pair:
 *   d = x - x_s, r2 = (dx dx + dy dy) + dz dz (every product and sum rounded: no fused multiply-add), r = sqrt(r2)   in double
 *   t = r (f / c) revolutions, u = t - rint(t)         in double: the phase is reduced before any rounding to float
 *   FUS_RAY_F64    s, c = sincospi(2 u); 1 / r; exp(-alpha r) (skipped when alpha == 0); e = exp(-alpha r) / r (c + i s);
 *                  w = q e; with the gradient v = (i k - alpha - 1/r) w and v d_j / r -- all in double
 *   FUS_RAY_MIXED  u, r, alpha r, q, d, k and alpha are rounded to float; sincospif, the reciprocal, the exponential
 *                  and every product above are in float
 * Both: the sums over s are kept in double, one target per thread, the sources taken in ascending order; the factor
 * -i f rho (= -i w rho / 2 pi) multiplies the finished sums in double.  The output is always double.
 * Chunks: where the targets are too few to fill the device (receivers, a small face) the sources are cut into
 * `chunks` contiguous ranges of ceil(nsrc / chunks) points, one workgroup per (256 targets, chunk); the partial sums go
 * to a workspace double[chunks][planes][ntgt] and a second kernel adds them in ascending chunk order (rmin: the
 * smallest).  No atomics: two identical calls return the same bits.  Option "rayleigh_chunks" forces the count (clipped to
 * nsrc); fus_rayleigh_plan reports out[0] = source chunks, out[1] = targets per workgroup, out[2] = kernel launches,
 * out[3] = workspace bytes.
 *   src_xyz  double[nsrc][3];  src_q double[nsrc][2] (re, im);  tgt_xyz double[ntgt][3]
 *   what     FUS_RAY_P is always implied; out = double[planes][ntgt], plane-major: P_re, P_im; with FUS_RAY_GRAD
 *            Px_re, Px_im, Py_re, Py_im, Pz_re, Pz_im; with FUS_RAY_RMIN the distance to the nearest source point
 *   space    FUS_HOST | FUS_DEVICE, for all four arrays
 * FUS_ERR_ARG, before anything is enqueued (out stays untouched): a null pointer; nsrc < 1 or ntgt < 1; a non-finite
 * coordinate or q (checked where the arrays are on the host); freq, c or rho not positive; alpha negative; unknown
 * bits in `what`, an unknown precision or space.  FUS_ERR_HIP names the bytes when the workspace or a staging buffer
 * cannot be allocated. */
enum { FUS_RAY_P = 1, FUS_RAY_GRAD = 2, FUS_RAY_RMIN = 4 };
enum { FUS_RAY_F64 = 0, FUS_RAY_MIXED = 1 };
int fus_rayleigh(fus_ctx* ctx, int64_t nsrc, const double* src_xyz, const double* src_q, int64_t ntgt,
                 const double* tgt_xyz, double freq, double c, double rho, double alpha, int what, int precision,
                 double* out, int space);
int fus_rayleigh_plan(fus_ctx* ctx, int64_t nsrc, int64_t ntgt, int what, int64_t out[4]);

/* ---- sources anywhere in the mesh: a source weight at any DOF -----------------------------------------------------
 * By default a DOF radiates only if it lies on a tag-1 boundary facet.  This call gives every DOF d a source weight
 * w_d of its own: its right-hand side gains  w_d g_d(t),  g_d the source function the model has (the default one,
 * fus_model_set_source's or fus_model_set_source_signals') -- exactly the term a tag-1 entry receives for its facet
 * weight.  A DOF that is also on the source boundary radiates with  facet weight + w_d.  The dg term of FUS_LOSSY /
 * FUS_WESTERVELT keeps the facet part only: a volume source s on the right of
 *   (1/(rho c^2)) p_tt - div((1/rho) grad p) - div((delta/(rho c^2)) grad p_t) = s
 * enters through the src term alone.  Units are the caller's:  w_d = s(x_d) (M(1) 1)_d  is a distributed source s under
 * GLL quadrature;  w_d = q phi_d(x0)  a point source of strength q at x0, phi_d(x0) the Lagrange basis values at the
 * located point (the transpose of what fus_model_sample evaluates).
 *   weights   T[ndofs] in caller numbering, host or device memory (`space`); finite, of either sign.  A non-finite value
 *             -> FUS_ERR_ARG, the model stays as it was.  NULL removes the weights: the model then computes, bit for bit,
 *             what a model that never had any computes.
 * Every call replaces the earlier weights (they do not accumulate) and puts amplitude / delay / duration / signals back
 * to the default source: set the weights first, then fus_model_set_source or fus_model_set_source_signals.  Legal once
 * the model's setup is finished (FUS_ERR_STATE before) and between steps; the state, the receivers and the monitor are
 * kept.  Cost: the call rebuilds the model's list of boundary entries on the host (every DOF with a source or absorbing
 * weight); no kernel changes, a step enqueues the same launches, and each weighted DOF costs what a boundary DOF costs.
 * Several ranks: each rank passes its own share of an interface DOF's weight (the shares of the sharers sum to the
 * source; the weight of a point source comes from the one rank whose cell was located), as each rank's facet term
 * rides in its own partial sum. */
int fus_model_set_source_weights(fus_model* model, const void* weights, int space);

/* ---- sampled drive signals: the source plays back tables of samples -----------------------------------------------
 * Instead of the windowed cosine, a DOF d with a source weight (facet weight and / or fus_model_set_source_weights')
 * and channel c = channel[d] >= 0 is driven by
 *   g_d(t)  = a_d S_c(t - tau_d)
 *   dg_d(t) = a_d S_c'(t - tau_d)                                 (the dg term of FUS_LOSSY / FUS_WESTERVELT)
 * S_c the cubic (Catmull-Rom) interpolant of the samples signals[c][j] at the times t_first + j ds: with
 * x = (t - t_first) / ds, j = floor(x), u = x - j, segment j uses the samples j-1 .. j+2, samples outside [0, nsamp)
 * counting as 0,
 *   S_c  = w_0 s_{j-1} + w_1 s_j + w_2 s_{j+1} + w_3 s_{j+2}
 *   w_0 = (-u + 2u^2 - u^3) / 2,  w_1 = (2 - 5u^2 + 3u^3) / 2,  w_2 = (u + 4u^2 - 3u^3) / 2,  w_3 = (-u^2 + u^3) / 2
 * and S_c' is the analytic derivative of the same cubic.  S_c passes through the samples, is C^1 on its support and
 * S_c = S_c' = 0 exactly before t_first - ds and after t_first + nsamp ds (start and end the signals at 0 and S_c is
 * C^1 everywhere).  There is no hidden factor: the signal stands in for the whole  C W(s) cos(w0 s)  of the default
 * source, including the scale = 2 of FUS_LOSSY / FUS_WESTERVELT with option "forms" = 0.  Evaluated in double for both
 * scalar types at the stage time the default source uses, rounded to T with the weight.
 *   nchan, nsamp       channels and samples per channel; nsamp >= 2
 *   t_first, ds        time of sample 0 and sample spacing, ds > 0
 *   signals            host, double[nchan][nsamp]; finite
 *   channel            host, int32[ndofs] in caller numbering, -1 = silent; NULL (only with nchan == 1) = channel 0
 *                      everywhere.  Values at DOFs without a source weight are ignored
 *   amplitude, delay   as in fus_model_set_source
 * Errors: those of fus_model_set_source, and channel[d] >= nchan (or < -1) at a DOF with a source weight, nsamp < 2,
 * ds <= 0, a non-finite sample -> FUS_ERR_ARG; the model stays as it was.  The table takes at most nchan nsamp 8 bytes
 * of device memory (channels no DOF uses are left out); if it cannot be allocated -> FUS_ERR_HIP naming the bytes, the
 * source stays as it was.  A successful fus_model_set_source (any arguments) leaves signal mode and frees the table.
 * Samples such as fenicsxfus_amd.source.waveform(..., scale=) produces reproduce the analytic source.  Cost: as the
 * per-entry source of fus_model_set_source, one small kernel launch per new stage time -- profile name "source_signal"
 * -- reading four samples per entry.  Legal once the model's setup is finished (FUS_ERR_STATE before) and between
 * steps; the state is kept.  Several ranks: every sharer of a DOF passes the same channel, amplitude and delay for it
 * and the same samples for that channel. */
int fus_model_set_source_signals(fus_model* model, int64_t nchan, int64_t nsamp, double t_first, double ds,
                                 const double* signals, const int32_t* channel, const void* amplitude, const void* delay,
                                 int space);

/* ---- relaxation absorption: power-law tissue absorption in the wave models -----------------------------------------
 * The wave models absorb thermoviscously only (delta0: alpha ~ f^2); soft tissue follows alpha ~ f^y with y = 1..1.3.
 * nrelax <= 4 relaxation processes with global angular relaxation frequencies w_nu > 0 (1/s) and per-cell strengths
 * a_nu >= 0 (1/s), added to any of the three models, fit such a law over a band (fenicsxfus_amd.absorption.fit_power_law):
 *   (1/(rho c^2)) [ u_tt + sum_nu a_nu (u_t - w_nu z_nu) ] = (the model's right-hand side),
 *   z_nu' = u_t - w_nu z_nu,   z_nu(0) = 0     (one memory variable per process and DOF)
 * A plane wave e^{i(w t - k x)} then has  k = (w/c) sqrt(1 + sum_nu a_nu / (w_nu + i w)),
 *   alpha = -Im k ~ (1/2c) sum_nu a_nu w^2 / (w_nu^2 + w^2).
 * c0 is the HIGH-frequency sound speed of such a medium; the low-frequency one is c0 / sqrt(1 + sum_nu a_nu / w_nu).
 * Per DOF the strength is A_nu = (M(a_nu/(rho c^2)) 1) / (M(1/(rho c^2)) 1), numerator and denominator summed over
 * the sharers before the division; 0 in the padding slots.
 * Time stepping: Strang splitting around every step of every RK order -- a relaxation sub-step of length dt/2, the RK
 * step as it is, a second sub-step of dt/2, then the receiver record and the monitor sample (they see the synchronised
 * state).  The sub-step is the trapezoidal rule on  v' = -sum A_nu (v - w_nu z_nu), z_nu' = v - w_nu z_nu  in closed
 * form: unconditionally stable, it never increases v^2/2 + sum_nu A_nu w_nu z_nu^2 / 2.  The absorption is second order
 * in dt.  Two launches of one streaming kernel per step (profile name "relax"), (3 nrelax + 2) sizeof(T) bytes per DOF
 * each, outside the graph of option "graph"; with relaxation off a step enqueues nothing new.
 *   fus_model_set_relaxation    omega: double[nrelax]; strength: host, T[nrelax][ncells] in the caller's cell order.
 *                               nrelax = 0 or strength = NULL switches relaxation off and frees the planes.  Otherwise
 *                               the memory variables start from 0.  Legal once the setup is finished (FUS_ERR_STATE
 *                               before) and between steps; u and v are kept.  nrelax outside 0..4, w_nu <= 0 or not
 *                               finite, a negative or non-finite strength -> FUS_ERR_ARG, the model stays as it was.
 *   fus_model_relaxation_get / _set   z_nu (nu = 0..nrelax-1), T[ndofs] in caller numbering, host or device: for
 *                               checkpoints and tests.  FUS_ERR_STATE while relaxation is off.  fus_model_init zeroes
 *                               the z_nu, fus_model_set leaves them alone.
 *   fus_model_relaxation_strength     A_nu as the sub-step reads it, T[ndofs] in caller numbering (diagnostics, tests)
 *   fus_model_relaxation_apply  one sub-step of length h >= 0 on the current state (what the stepping entries call)
 * Several ranks: on a single object with neighbours under RCCL fus_model_set_relaxation is collective (it sums the
 * nrelax + 1 lumped vectors over the sharers).  The members of an in-process group call fus_model_set_relaxation each
 * and then fus_group_relaxation_finish once; stepping a member before that -> FUS_ERR_STATE.  A model with neighbours
 * under the external transport -> FUS_ERR_STATE (no entry points for the sums there).  The sub-step itself needs no
 * exchange: the sharers of a DOF hold identical v and identical A_nu. */
int fus_model_set_relaxation(fus_model* model, int nrelax, const double* omega, const void* strength /* T[nrelax][ncells] */);
int fus_model_relaxation_get(fus_model* model, int nu, void* out, int space);
int fus_model_relaxation_set(fus_model* model, int nu, const void* in, int space);
int fus_model_relaxation_strength(fus_model* model, int nu, void* out, int space);
int fus_model_relaxation_apply(fus_model* model, double h);
int fus_group_relaxation_finish(fus_model** models, int n);

/* ---- absorbing layers: a split-step sponge in the wave models ------------------------------------------------------
 * The first-order condition on tag-2 facets (u_t / c) is exact at normal incidence and reflects
 * (1 - cos th) / (1 + cos th) of the amplitude at the angle th: 17 % at 45 degrees, 33 % at 60.  A steered or focused
 * beam and above all a point source meet the faces at every angle.  With a damping rate sigma(x) >= 0 (1/s) per DOF,
 * zero outside the layers, any of the three models solves
 *   (d/dt + sigma)^2 u = (the model's right-hand side),   i.e.   u_t = v - sigma u,   v_t = RHS(u, v) - sigma v
 * A plane wave e^{i(w t - k.x)} then has k = (w - i sigma) / c in its own direction, whatever the direction: it decays
 * as e^{-sigma s / c} along its path, without dispersion and independent of angle and frequency (Cerjan's sponge in
 * continuous form).  The local impedance mismatch comes from the gradient of sigma alone, which the profile keeps small.
 * For sigma(d) = sigma_max (d / L)^n over the thickness L the round-trip amplitude reflection off whatever lies behind
 * the layer is R = exp(-2 sigma_max L / ((n + 1) c)); a design R gives sigma_max = (n + 1) c ln(1 / R) / (2 L)
 * (fenicsxfus_amd.sponge.layer_sigma builds such profiles from DOF coordinates).
 * Time stepping: Strang splitting around every step of every RK order, outside the relaxation sub-steps -- sponge(dt/2),
 * relaxation(dt/2), the RK step as it is, relaxation(dt/2), sponge(dt/2), then the receiver record and the monitor sample
 * (they see the synchronised state).  The sub-step solves u' = -sigma u, v' = -sigma v exactly: both fields, and with
 * relaxation on the memory variables z_nu, are multiplied by g = exp(-sigma h), formed in double and rounded once to T.
 * A scaling: unconditionally stable, it increases no quadratic energy, the stable_dt rules are untouched, and where
 * sigma = 0 a DOF keeps its bits.  With constant sigma the linear models with relaxation commute with the scaling: a run
 * with the sponge is exactly e^{-sigma t} times the run without it.
 * Inside a layer v holds u_t + sigma u, not u_t; outside nothing changes.  The first-order condition on the outer face,
 * acting on that v, is the matched condition of the damped medium: keep tag 2 on the faces behind the layers.  The
 * nonlinear terms of the Westervelt model see that v too; amplitudes in a layer are small and nothing corrects for it.
 * Two launches of one streaming kernel per step (profile name "sponge") over the tiles -- runs of 256 16-byte vectors of
 * the internal vector -- that hold a nonzero sigma, (2 nrelax + 5) sizeof(T) bytes per DOF of those tiles, outside the
 * graph of option "graph"; DOFs of other tiles are neither read nor written, and with the sponge off a step enqueues
 * nothing new.
 *   fus_model_set_sponge    sigma: T[ndofs] in caller numbering, host or device.  NULL or an all-zero sigma switches the
 *                           sponge off and frees the plane and the tile list.  Legal once the setup is finished
 *                           (FUS_ERR_STATE before) and between steps; u, v and the z_nu are kept.  A negative or
 *                           non-finite value -> FUS_ERR_ARG, the model stays as it was.  Legal before or after
 *                           fus_model_set_relaxation.
 *   fus_model_sponge_get    sigma back, T[ndofs] in caller numbering.  FUS_ERR_STATE while the sponge is off.
 *   fus_model_sponge_apply  one sub-step of length h >= 0 on the current state (what the stepping entries call).
 *                           h < 0 or not finite -> FUS_ERR_ARG; sponge off, or neither fus_model_init nor fus_model_set
 *                           before it -> FUS_ERR_STATE.
 *   fus_model_sponge_info   DOFs with sigma > 0, listed tiles, tiles of the whole internal vector (any pointer may be NULL)
 * Several ranks: nothing is summed over sharers, so the sub-step needs no exchange and no group finish call, and it
 * works under RCCL, in an in-process group and under the external transport alike.  The contract: the sharers of a DOF
 * pass the same sigma (a profile computed from coordinates does).  It is not checked across ranks. */
int fus_model_set_sponge(fus_model* model, const void* sigma /* T[ndofs], 1/s, caller numbering; NULL: off */, int space);
int fus_model_sponge_get(fus_model* model, void* out, int space);
int fus_model_sponge_apply(fus_model* model, double h);
int fus_model_sponge_info(fus_model* model, int64_t* ndofs_active, int64_t* ntiles_active, int64_t* ntiles_total);

/* ---- bioheat: Pennes equation and CEM43 thermal dose on the operator's mesh ---------------------------------------
 * What a focused-ultrasound user computes from the pressure maps: the temperature rise the beam causes and the thermal
 * dose it leaves.  (The reference has no thermal model; this section replaces nothing there.)
 *
 * State: the temperature RISE theta = T - t_base over a uniform baseline t_base (arterial and initial temperature,
 * degrees C); the rise and not the temperature, so that FUS_F32 objects do not lose a 0.01 K increment against 37.
 *   rho C dtheta/dt = div(k grad theta) - W theta + Q,     natural (insulating) boundaries unless
 *                                                          fus_thermal_set_boundary sets others (below)
 * Per-cell coefficients, host T[ncells] in caller cell numbering: conductivity k >= 0 (W/m/K), rho_c > 0 (J/m^3/K),
 * perfusion W = w_b rho_b C_b >= 0 (W/m^3/K; NULL = 0).  On the GLL-collocated space of the wave models, with the
 * library's K(c) and M(c) (u^T K(1) u = integral of |grad u|^2):
 *   m_C = M(rho_c) 1     m_W = M(W) 1     h = (M(q_coef) 1) .* q                  (all diagonal)
 *   dtheta/dt = f(theta) = ( K(-k) theta - m_W .* theta + sigma h ) ./ m_C
 * q is a nodal field, q_coef a per-cell factor (NULL = 1), h the heat load in W per DOF, sigma the scalar heat_scale of a
 * fus_thermal_steps call (duty cycle; 0 = cooling).  Acoustic heating Q = 2 alpha p_rms^2 / (rho c): q = p_rms^2,
 * q_coef = 2 alpha / (rho c), alpha the amplitude absorption in Np/m at the source frequency.
 * Time stepping: classical RK4, a = (0, 1/2, 1/2, 1), b = (1/6, 1/3, 1/3, 1/6); f has no explicit time dependence.
 * Per stage the operator's two launches and one streaming kernel (profile name "thermal").
 * Dose: double[ndofs] for both scalar types.  After each completed step of size dt that ends in theta_n, in double:
 *   T = t_base + theta_n;   c = 1 if T >= 43 else 2;   D += (dt / 60) * exp2(-c * (43 - T))
 * -- CEM43 in minutes after Sapareto and Dewey, a rectangle rule on the end-of-step temperature, added in the last
 * stage's pass (the dose plane is read and written once per step).
 * Stable step: RK4 needs dt <= 2.785 / lambda_max of m_C^-1 (K(k) + diag m_W).  fus_thermal_lambda_max runs a power
 * iteration from x_d = 1 + 0.5 sin(37 d + 1) (d = caller DOF number): iters times y = (K(k) x + m_W .* x) ./ m_C,
 * rho = (x . (m_C .* y)) / (x . (m_C .* x)), x = y / sqrt(y . (m_C .* y)); it returns the last rho, which never exceeds
 * lambda_max (20 iterations reach about 0.97 of it on small meshes; dt = 2 / rho_20 stays inside the limit while
 * rho_20 >= 0.72 lambda_max).  Setup-time work: the dot products are taken on the host from the pulled vector.
 * Super-time-stepping (fus_thermal_steps_sts): the RK4 step is bound by the diffusion limit alone, which grows like
 * P^4 / h^2 while the temperature field stays smooth.  The stabilised Runge-Kutta-Legendre scheme of second order (RKL2:
 * Meyer, Balsara and Aslam, J. Comput. Phys. 257, 2014) takes s stages of one operator application each and is stable
 * for dt lambda_max <= beta_s = (s^2 + s - 2) / 2; the discrete operator is symmetric negative semi-definite in the m_C
 * inner product, so the negative real axis is all that matters.  With b_0 = b_1 = b_2 = 1/3,
 * b_j = (j^2 + j - 2) / (2 j (j + 1)), a_j = 1 - b_j, w1 = 4 / (s^2 + s - 2), mut_1 = b_1 w1 and, for j = 2..s,
 * mu_j = (2j - 1)/j b_j / b_{j-1}, nu_j = -(j - 1)/j b_j / b_{j-2}, mut_j = mu_j w1, gat_j = -a_{j-1} mut_j:
 *   Y_0 = theta,  F_0 = f(Y_0),  Y_1 = Y_0 + mut_1 dt F_0
 *   Y_j = mu_j Y_{j-1} + nu_j Y_{j-2} + (1 - mu_j - nu_j) Y_0 + mut_j dt f(Y_{j-1}) + gat_j dt F_0,    theta <- Y_s
 * Per stage the operator's two launches and one streaming kernel (profile name "thermal_sts"); one more state-sized
 * vector (F_0) than RK4, allocated by the first fus_thermal_steps_sts call.  stages lies in 2..32, the range over which
 * the stability polynomial and the rounding behaviour of the recurrence have been checked.  The steps are long against
 * the dose rate's growth, so this path integrates the dose by the TRAPEZOID rule, after each step from theta_old to
 * theta_new, in double:   D += (dt / 120) * (R(T_old) + R(T_new)),   R(T) = exp2(-c * (43 - T)),   c = 1 if T >= 43 else 2.
 * RK4 steps and super-steps of any stage count may follow each other on one object.
 * fus_thermal_stable_dt: stages = 0 gives the RK4 step 2 / rho_iters; stages = s in 2..32 gives 0.72 beta_s / rho_iters,
 * the same margin (0.72 = 2 / 2.785) and safe under the same condition, rho_iters >= 0.72 lambda_max.
 * Boundary conditions (fus_thermal_set_boundary): every face is insulating until a DOF is declared
 *   fixed        theta = theta_D, a given nodal rise over t_base (a cut face in tissue at body temperature: 0), or
 *   convective   -k dtheta/dn = h_c (theta - theta_ext): h_c >= 0 in W/m^2/K, theta_ext the coolant's rise over t_base
 *                (negative for cold water).
 * Both are diagonal on the collocated space.  The caller passes per-DOF host arrays in its own numbering: a mask `fixed`
 * with the values fixed_rise, and conv_diag = m_H = sum over the convective facets of h_c |J_f| w_a w_b -- what
 * fus_facet_diag returns for cellcoef = h_c, summed over the faces -- with conv_rise = theta_ext.  With r = m_H .* theta_ext,
 * formed in double and rounded to T once,
 *   f(theta) = ( K(-k) theta - m_W .* theta - m_H .* theta + r + sigma h ) ./ m_C     at the free DOFs
 *   f(theta) = 0,  theta = theta_D                                                   at the fixed DOFs
 * r is NOT scaled by sigma: the coolant keeps working while the beam is off.  A DOF both fixed and convective is fixed; the
 * heat load at a fixed DOF is ignored; the dose keeps accumulating there from the fixed temperature.  The fixed values hold
 * exactly through every step of either scheme.  fus_thermal_lambda_max and fus_thermal_stable_dt then work on
 * m_C^-1 (K(k) + diag(m_W + m_H)) with the rows and columns of the fixed DOFs removed (x_d = 0 and y = 0 there), which is
 * still symmetric and non-negative in the m_C inner product, so both step rules apply unchanged -- and are needed: a
 * water-cooled face (h_c = 5000) puts dt max(m_H / m_C) above 2 at the insulating operator's step.
 * Cost: the lists are sparse, proportional to the surface.  Convective DOFs add one small launch per operator application
 * (profile name "thermal_bc"); fixed DOFs add none to an RK4 step (the stage kernels read a copy of 1 / m_C that is zero
 * there, as it is in the padding slots) and one per RKL2 step, which puts the values back after the stages' weighted sums
 * (profile name "thermal_fix", also counted when fus_thermal_init / fus_thermal_set / fus_thermal_set_boundary /
 * fus_thermal_lambda_max write them).  With no boundary set, or after clearing it, a step enqueues exactly the launches of
 * an object that never had one, with the same arguments.
 *
 *   fus_thermal_create   on an existing operator object, also one created with "fields" = 2; several thermal objects and wave
 *                        models may share one op and run in turns on the context's stream
 *   fus_thermal_init     theta = 0 (fixed DOFs: their values), D = 0
 *   fus_thermal_set      which = FUS_TH_RISE: T[ndofs] (fixed DOFs take their values again); FUS_TH_DOSE: double[ndofs];
 *                        caller numbering, `space`
 *   fus_thermal_get      FUS_TH_RISE, FUS_TH_HEAT (= h): T[ndofs]; FUS_TH_DOSE: double[ndofs]; FUS_TH_DAMAGE and
 *                        FUS_TH_PERFUSION: "perfusion response and damage" below
 *   fus_thermal_set_heat q: T[ndofs], q_coef: T[ncells] or NULL (= 1), both in `space`; q == NULL: h = 0
 *   fus_thermal_set_heat_from_monitor   h from the field monitor of a wave model on the SAME fus_op, without leaving
 *                        the device: q = Q / n from the monitor's sum-of-squares plane and sample count, formed in
 *                        double (the RMS map is never rounded through a square root), q_coef = 2 alpha / (rho c) with
 *                        the model's rho0 and c0; absorption = alpha, host T[ncells], >= 0.  The monitor keeps sampling
 *   fus_thermal_set_heat_from_harmonics   h from the monitor's harmonics, each with its own absorption ("per-harmonic
 *                        heat load" below); preconditions and errors as fus_thermal_set_heat_from_monitor
 *   fus_thermal_steps    nsteps RK4 steps of size dt with heat_scale sigma
 *   fus_thermal_steps_sts   nsteps RKL2 steps of `stages` stages each; states and argument checks as fus_thermal_steps,
 *                        and FUS_ERR_ARG for stages outside 2..32
 *   fus_thermal_stable_dt   lambda_max(iters) turned into a step for RK4 (stages = 0) or RKL2 (stages in 2..32)
 *   fus_thermal_set_boundary   replaces any boundary set before; all arrays NULL clears it.  Before or after
 *                        fus_thermal_init; theta at the fixed DOFs is overwritten at once.  fus_thermal_get(FUS_TH_HEAT)
 *                        is unchanged
 *   fus_thermal_boundary_info  the number of fixed and of convective DOFs in force (either pointer may be NULL)
 * Errors; argument and call-sequence errors (FUS_ERR_ARG, FUS_ERR_STATE) are found before anything is enqueued and leave the
 * state and the heat load as they were.  A FUS_ERR_HIP inside fus_thermal_steps returns at the failing step: the steps before
 * it have been applied and the stream is not synchronised.  FUS_ERR_ARG: null arguments; rho_c <= 0, a negative or
 * non-finite k, W, alpha or conv_diag entry; a non-finite fixed_rise where fixed is set or conv_rise where conv_diag > 0;
 * conv_rise without conv_diag (these leave the previous boundary in force); dt <= 0; iters < 1; stages outside 2..32 (fus_thermal_stable_dt: 0 or 2..32); a fus_model on
 * another fus_op than the thermal object's.  FUS_ERR_STATE:
 * steps before fus_thermal_init / fus_thermal_set; fus_thermal_stable_dt on a zero operator (k = 0 and W = 0 everywhere:
 * every step is stable); fus_thermal_set_heat_from_monitor while the model's monitor is off,
 * has no sample, or watches FUS_V; an op on which fus_op_set_neighbours was called in a context without a transport
 * (below); a call that needs sums which still wait for fus_group_thermal_finish; a single-object call that exchanges, on
 * a member of an in-process group.
 * Several ranks: fus_thermal_create accepts an op with neighbours when the context has a transport of the library's own,
 * an RCCL communicator (fus_comm_init) or an in-process group (fus_comm_init_local).  Without one -- a plain context, or
 * one set up for the external transport, whose entry points do not cover the thermal model -- it fails with FUS_ERR_STATE
 * before anything is allocated.  An interface DOF (one that other ranks hold too) then works as in the wave models: every
 * rank forms its own total, the totals are exchanged, and every sharer adds them in ascending rank order, so that all
 * of them hold the same bits.
 *   Setup sums.  m_C, m_W and the heat weight M(q_coef) 1 are such sums, formed before their first use: 1 / m_C after
 *   the sum of m_C, h = (M(q_coef) 1) .* q after the sum of the weight.  The convective diagonal m_H and r are NOT summed:
 *   like the wave models' boundary weights each rank's part rides in its partial operator result.  A DOF is fixed if any
 *   sharer fixes it, at the mean of the values the fixing sharers gave (callers are expected to give the same one): sums
 *   of the 0/1 flags and of flag * value; a sharer drops its convective entry on a DOF another rank fixed.
 *   Under RCCL fus_thermal_create, fus_thermal_set_heat (q != NULL), fus_thermal_set_heat_from_monitor and
 *   fus_thermal_set_boundary are collective and exchange at once.  In an in-process group they leave the sums pending, and
 *   fus_group_thermal_finish performs whatever is pending on the members: idempotent, and legal again after a later
 *   set_heat or set_boundary (a new boundary on one member makes all members agree again; a heat load must be set on
 *   all members or none).  While something is pending fus_thermal_init, _set, _steps, _steps_sts, _lambda_max and
 *   _stable_dt fail with FUS_ERR_STATE.
 *   The step.  Each stage is split as the wave models' stages are.  First half: the operator's two launches and the
 *   convective term leave this rank's total in b, also at the interface DOFs; these are packed into the send buffer
 *   (profile name "halo").  Second half: the streaming kernel runs over the DOFs no other rank holds -- the first
 *   n_int_pad + n_if_start_pad slots, a multiple of 16 -- while the exchange is in flight, and after the receive one
 *   thread per interface DOF adds the totals in order and applies the same stage update, dose included (profile name
 *   "thermal_if").  Under RCCL fus_thermal_steps / _steps_sts do this as collective calls; the members of an in-process
 *   group are advanced in lock-step by fus_group_thermal_steps (stages = 0: RK4; 2..32: RKL2), which checks arguments
 *   and states of every member before anything is enqueued; the single-object calls fail there with FUS_ERR_STATE.
 *   Without neighbours a step enqueues exactly the launches of the one-rank path, with the same arguments.
 *   Step rule.  Every rank starts from 1 + 0.5 sin(37 d + 1) over its OWN DOF numbers; one ordered sum makes the start
 *   identical on the sharers of a DOF (an interface DOF carries the sum of its sharers' values), the fixed DOFs are
 *   zeroed.  Every operator result is exchanged; the three inner products count a DOF on the rank that owns it -- the
 *   lowest rank that holds it -- and are added over the ranks (ncclAllReduce, or on the host across the group) before the
 *   quotient is formed, so every rank gets the same double.  fus_group_thermal_lambda_max / _stable_dt for a group.
 *   One fus_op serves EITHER thermal steps OR wave steps at a time: both use its send / receive buffers and d_partial
 *   (for d_partial this was the rule already); calls in turns on the context's stream are fine, concurrent ones are not.
 *   Not covered: the external transport, graph capture of thermal steps, overlapping the exchange with part of the block
 *   kernel ("overlap_blocks" has no effect here).
 * Per-harmonic heat load (fus_thermal_set_heat_from_harmonics).  Tissue absorption grows with frequency, so the energy a
 * nonlinear beam has moved into its harmonics heats faster than alpha at the source frequency times p_rms^2 says.  Let n be
 * the monitor's sample count, C_k and S_k its cosine and sine accumulators (COS_k = 2 C_k / n, SIN_k = 2 S_k / n), K = nharm
 * the number of harmonics asked for and alpha_k[e] >= 0 the amplitude absorption in Np/m of cell e at k times the source
 * frequency:
 *   a_k = (2 / n^2) (C_k^2 + S_k^2) = (COS_k^2 + SIN_k^2) / 2      the mean square of harmonic k
 *   m_k = M(2 alpha_k / (rho c)) 1                                 the model's own c0, rho0 per cell, as the rms path uses them
 *   h   = sum_{k = 1..K} m_k .* a_k                                W per DOF
 * The sum over k is carried in double for both scalar types, in ascending k, as sum_k (double) m_k (C_k^2 + S_k^2), then
 * scaled by 2 / n^2 and rounded to T once: the fp32 error does not grow with K.  The mean (DC) term and everything above
 * harmonic K carry NO heat; with all alpha_k equal, h is the rms path's load of the signal minus its mean and minus
 * that residual.  a_k is the mean square of harmonic k only over a window of whole source periods sampled uniformly with
 * more than 2 K samples per period (fenicsxfus_amd.monitor.whole_period_window); the library does not check the window.
 *   absorption   host T[nharm][ncells], caller cell numbering, row k - 1 = alpha_k
 *   nharm        1..8 (else FUS_ERR_ARG), at most the monitor's own nharm (else FUS_ERR_STATE); fewer uses harmonics 1..nharm
 * FUS_ERR_ARG: a null argument, a model on another fus_op, nharm outside 1..8, a negative or non-finite entry in any row.
 * FUS_ERR_STATE: the monitor is off, watches FUS_V, has no sample, or holds fewer harmonics.  All are found before
 * anything is enqueued; the heat load stays as it was and the monitor's accumulators are never altered.
 * Device work, at setup time: per harmonic the lumped weight (the operator's two launches) and one streaming launch over
 * one double scratch plane; fus_thermal_set_heat and fus_thermal_set_heat_from_monitor enqueue what they always did.
 * Several ranks: a_k has the same bits on every sharer of a DOF because the states do, so the sharers' parts of h itself,
 * sum_k m_k(part) .* a_k rounded to T, are summed in one ordered exchange (not K weights), and all sharers end with the
 * same bits.  Under RCCL the call is collective and exchanges at once; in an in-process group the part waits for
 * fus_group_thermal_finish like any heat load (on every member or none, and of the same kind on all of them);
 * fus_thermal_set_heat(q = NULL) drops it.
 * Perfusion response and damage (fus_thermal_set_response, fus_thermal_set_damage).  Blood flow rises several-fold under
 * mild heating and stops for good where the tissue is coagulated; fus_thermal_set_response lets the perfusion term follow
 * the temperature and the dose, one law per thermal object (tissue differences stay in the per-cell W).  With
 * T = t_base + (double) theta and the dose D of a DOF, in double for both scalar types, every operation rounded by itself:
 *   P(T)   1 if nknots == 0; else factor[0] for T <= temp[0], factor[n-1] for T >= temp[n-1], and between them, with j
 *          the largest index with temp[j] <= T:
 *            factor[j] + (factor[j+1] - factor[j]) * ((T - temp[j]) / (temp[j+1] - temp[j]))
 *   S(D)   1 if dose_hi <= 0 (no shutdown); else 1 for D <= dose_lo, 0 for D >= dose_hi,
 *          (dose_hi - D) / (dose_hi - dose_lo) between them; dose_lo == dose_hi > 0 is a step (1 at D == dose_lo)
 *   phi = P * S,      m_Weff = (T)((double) m_W * phi)
 * phi is taken from the state at the START of a step, (theta_n, D_n), and held through all stages of that step, for RK4
 * and for every RKL2 stage count alike: within a step the operator is the linear, symmetric one both step rules assume,
 * and f reads m_Weff where it read m_W.
 *   nknots 0..8; temp strictly ascending and finite, degrees C; factor finite and >= 0; 0 <= dose_lo <= dose_hi (finite),
 *   or dose_hi <= 0.  Anything else is FUS_ERR_ARG, and the response stays as it was.  nknots == 0 with dose_hi <= 0
 *   clears the response.  Legal before or after fus_thermal_init and between steps; the state is kept.  On an object
 *   without perfusion the call is accepted and changes no result.
 * Step rule: fus_thermal_lambda_max and fus_thermal_stable_dt (and the group forms) then work on
 * m_C^-1 (K(k) + diag(phi_max m_W + m_H)), phi_max = max_j factor[j] (1 without knots).  The difference to the operator of
 * any phi in force, diag((phi_max - phi) m_W), is a non-negative diagonal, and adding one cannot lower an eigenvalue of the
 * symmetric pencil: the quotient's lambda_max bounds that of every state from above, so the step taken from it is stable
 * throughout.  Like fus_thermal_set_boundary, fus_thermal_set_response must therefore precede fus_thermal_stable_dt.
 * Damage: fus_thermal_set_damage(A, Ea) switches on the Arrhenius integral Omega, double[ndofs] for both scalar types,
 * zeroed by the call that switches it on and by fus_thermal_init.  A in 1/s, Ea in J/mol, both positive and finite (else
 * FUS_ERR_ARG); A == 0 switches the damage off and frees its memory; new constants on a running integral keep its value.
 * After every completed step of EITHER scheme, from theta_old to theta_new, in double, every operation rounded by itself:
 *   r(T) = exp(lnA - Ea / (R * (T + 273.15))),   R = 8.314462618,   lnA = log(A) taken once on the host
 *   Omega += (dt / 2) * (r(T_old) + r(T_new))                        (trapezoid rule)
 * Fixed DOFs accumulate damage from their fixed temperature, as the dose does.
 *   fus_thermal_get / _set   FUS_TH_DAMAGE: double[ndofs], FUS_ERR_STATE while the damage is off
 *   fus_thermal_get          FUS_TH_PERFUSION: T[ndofs], read only: the plane m_Weff the next step will use -- m_W itself
 *                            while no response is set, zeros without perfusion
 * Cost: while neither is set a step enqueues exactly the launches of an object that never had them, with the same
 * arguments (the stage kernels keep reading m_W).  With either set, a step gains ONE streaming launch (profile name
 * "thermal_response") after its last stage -- on several ranks after the interface kernel, on the RKL2 path after
 * "thermal_fix".  It reads theta_{n+1}, D_{n+1} and m_W, and for the damage Omega and a stored double plane with
 * r(T_{n+1}) of the step before; it writes m_Weff for the next step, Omega and that plane: the stage kernels only get
 * another pointer.  The knot table travels in the kernel arguments.  A steps call (or a read of FUS_TH_PERFUSION) starts
 * with one more such launch when fus_thermal_init, _set, _set_boundary, _set_response or _set_damage (or a
 * fus_group_thermal_finish that had work) came since the last step: it forms m_Weff and the stored rate from the state as
 * it stands and leaves Omega alone.
 * Several ranks: every operand of phi and r (the states, D, the summed m_W) has the same bits on all sharers of a DOF, so
 * the launch covers all of a rank's slots without an exchange and the sharers stay identical; under RCCL nothing becomes
 * collective.  fus_group_thermal_steps, _lambda_max and _stable_dt check before anything is enqueued that all members
 * carry the same response and damage parameters (else FUS_ERR_STATE). */
typedef struct fus_thermal fus_thermal;
enum { FUS_TH_RISE = 0, FUS_TH_DOSE = 1, FUS_TH_HEAT = 2, FUS_TH_DAMAGE = 3, FUS_TH_PERFUSION = 4 };
int fus_thermal_create(fus_ctx* ctx, fus_op* op, const void* conductivity, const void* rho_c,
                       const void* perfusion /* NULL = 0 */, double t_base, fus_thermal** thermal);
int fus_thermal_destroy(fus_thermal* thermal);
int fus_thermal_init(fus_thermal* thermal);
int fus_thermal_set(fus_thermal* thermal, int which, const void* in, int space);
int fus_thermal_get(fus_thermal* thermal, int which, void* out, int space);
int fus_thermal_set_heat(fus_thermal* thermal, const void* q, const void* q_coef, int space);
int fus_thermal_set_heat_from_monitor(fus_thermal* thermal, fus_model* model, const void* absorption /* T[ncells], Np/m */);
int fus_thermal_set_heat_from_harmonics(fus_thermal* thermal, fus_model* model, int nharm,
                                        const void* absorption /* T[nharm][ncells], Np/m, row k - 1 = harmonic k */);
int fus_thermal_lambda_max(fus_thermal* thermal, int iters, double* lambda);
int fus_thermal_steps(fus_thermal* thermal, double dt, int64_t nsteps, double heat_scale);
int fus_thermal_steps_sts(fus_thermal* thermal, double dt, int64_t nsteps, double heat_scale, int stages);
int fus_thermal_stable_dt(fus_thermal* thermal, int iters, int stages, double* dt);
/* host arrays, caller DOF numbering; any of them may be NULL (fixed == NULL: no fixed DOF; conv_diag == NULL:
 * no convective DOF; fixed_rise / conv_rise == NULL: 0).  Replaces any boundary set before; all NULL clears it. */
int fus_thermal_set_boundary(fus_thermal* thermal, const uint8_t* fixed /* [ndofs], != 0: fixed */,
                             const void* fixed_rise /* T[ndofs], read where fixed */,
                             const void* conv_diag /* T[ndofs] = m_H >= 0 */, const void* conv_rise /* T[ndofs] */);
int fus_thermal_boundary_info(fus_thermal* thermal, int64_t* nfixed, int64_t* nconvective);
int fus_thermal_set_response(fus_thermal* thermal, int nknots /* 0..8 */, const double* temp /* [nknots], degrees C */,
                             const double* factor /* [nknots], >= 0 */, double dose_lo, double dose_hi /* <= 0: no shutdown */);
int fus_thermal_set_damage(fus_thermal* thermal, double A /* 1/s; 0: off */, double Ea /* J/mol */);
/* the members of an in-process group, one thermal object per rank, in any order */
int fus_group_thermal_finish(fus_thermal** thermals, int n);
int fus_group_thermal_steps(fus_thermal** thermals, int n, double dt, int64_t nsteps, double heat_scale,
                            int stages /* 0: RK4; 2..32: RKL2 */);
int fus_group_thermal_lambda_max(fus_thermal** thermals, int n, int iters, double* lambda);
int fus_group_thermal_stable_dt(fus_thermal** thermals, int n, int iters, int stages, double* dt);

int fus_group_finish_setup(fus_model** models, int n);
int fus_group_rk4_steps(fus_model** models, int n, double t0, double dt, int64_t nsteps);

/* ---- external transport ---------------------------------------------------------------------
 * For callers that move the interface values themselves -- GPU-aware MPI in the reference's setting
 * (its scatter_fwd/scatter_rev, Linear.hpp:196-206, are MPI neighbourhood exchanges) -- instead of
 * the built-in RCCL exchange.  fus_set_option(ctx, "external_transport", 1), then
 * fus_comm_init(ctx, rank, nranks, NULL), fus_op_create, fus_op_set_neighbours, fus_model_create.
 *   fus_op_halo_layout   neighbours in the order of the buffers: rank, number of values, offset (values)
 *   fus_op_halo_buffers  device pointers of the send / receive buffers (element type T) and their length;
 *                        neighbour k sends send[off_k .. off_k + count_k) and receives into the same
 *                        range of recv
 * Setup (once): for k in [0, fus_model_setup_count): fus_model_setup_pack(k) -> exchange ->
 * fus_model_setup_unpack(k); then fus_model_setup_finish, fus_model_init.
 * Every RK stage i of a step at time t: fus_model_stage_begin(i, t, dt) -> exchange ->
 * fus_model_stage_end(i, t, dt).  *_pack / stage_begin return with the send buffer complete; the
 * receive buffer must be complete when *_unpack / stage_end are called.  Every sharer adds the ranks'
 * values in ascending rank order, so all of them end with identical bits. */
int fus_op_halo_layout(fus_op* op, int* nneigh, int32_t* ranks, int64_t* counts, int64_t* offsets);
int fus_op_halo_buffers(fus_op* op, void** send_dev, void** recv_dev, int64_t* nvalues);
int fus_model_setup_count(fus_model* model);
int fus_model_setup_pack(fus_model* model, int k);
int fus_model_setup_unpack(fus_model* model, int k);
int fus_model_setup_finish(fus_model* model);
int fus_model_stage_begin(fus_model* model, int stage, double t, double dt);
int fus_model_stage_end(fus_model* model, int stage, double t, double dt);

/* ---- measurement -----------------------------------------------------------------------------
 * HIP-event timing of the library's own kernels on the stream they run on.  Names:
 * "stiffness" (block operator kernel), "shared" (shared-DOF reduction), "stage" (fused RK stage
 * update), "boundary", "halo", "monitor" (field-monitor sample), "source" (per-entry source waveform), "source_signal" (the
 * same for sampled drive signals),
 * "thermal" (bioheat stage update; its operator passes count under "stiffness" and "shared"), "thermal_sts" (the
 * same for a super-time-stepping stage), "thermal_bc" (convective surface term, once per operator application of a
 * bioheat object with convective DOFs), "thermal_fix" (writes of the fixed values), "thermal_if" (bioheat stage update of
 * the interface DOFs on several ranks; the pack of their totals counts under "halo"), "thermal_response" (perfusion
 * response and damage, once per step of a bioheat object that has either).  total_ms/count accumulate since the last enable.
 * on = 1: every kernel; on = 2: only the block operator kernel ("stiffness", and "stiffness_if" when
 * the interface blocks are launched separately) -- an event record drains the queue between two
 * kernels, so timed runs use 2 (bench.py) and take the full breakdown in a separate pass.  Option
 * "profile_sample" = k (fus_set_option, default 1): level 2 puts its events around every k-th launch of the
 * block operator kernel only (k = 5 samples the four RK4 stage kinds equally and costs a timed run 0.3 % instead
 * of 1.7 %); fus_profile_get then returns the time and the count of the sampled launches. */
int fus_profile_enable(fus_ctx* ctx, int on);
int fus_profile_get(fus_ctx* ctx, const char* name, double* total_ms, int64_t* count);
/* Measured streaming bandwidth of the device (16-byte non-temporal copy of nbytes, one vector per
 * thread; bytes read + bytes written per second, best of reps launches, GB/s): reported beside the
 * roofline fractions. */
int fus_measure_bandwidth(fus_ctx* ctx, int64_t nbytes, int reps, double* gbps);

/* Host-only layout builder (no device needed): runs the block partitioner / DOF renumbering on
 * a dofmap and returns statistics as fus_op_info does; used by the CPU test-suite. */
int fus_layout_check(int P, int64_t ncells, int64_t ndofs, const int32_t* tensor_dofmap,
                     const double* centroids /* [ncells*3] */, int block_elems, int waves,
                     int64_t out[8]);
/* The same for tdim = 2 | 3 and with the optional mask of DOFs other ranks hold as well
 * (force_shared, uint8[ndofs] or NULL): those DOFs are classified shared and the blocks touching
 * them come first in the layout (fus_op_set_neighbours does this on the device path). */
int fus_layout_check_ex(int tdim, int P, int64_t ncells, int64_t ndofs, const int32_t* tensor_dofmap,
                        const double* centroids, int block_elems, int waves,
                        const uint8_t* force_shared, int64_t out[8]);

#ifdef __cplusplus
}
#endif
#endif
