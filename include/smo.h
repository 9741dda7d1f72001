/*
 * smo.h — C-ABI of the MI355X-native forward/adjoint spectral-solve hot path of SphereManOpt.
 *
 * The reference is pure Python; its optimiser (Sphere_Grad_Descent.py:692) reaches the hot path only through
 * three callbacks  f / Grad_f / Inner_Product  (SURVEY.md section 8b).  This header is what those callbacks
 * bind to (ctypes stub: INTEGRATION.md; shipped binding: spheremanopt_amd/_capi.py):
 *
 *   smo_create    <- per-call solver construction the reference repeats inside every f / Grad_f:
 *                    FWD_Solve_Build_Lin   FWD_Solve_SH23.py:279-332, FWD_Solve_KDyn.py:362-450,
 *                    LBVP build            FWD_Solve_SHB23.py:563-587;  GEN_BUFFER (snapshot stack)
 *                    FWD_Solve_SH23.py:238-272, FWD_Solve_KDyn.py:319-355, FWD_Solve_SHB23.py:270-314
 *   smo_forward   <- FWD_Solve_IVP_Lin      FWD_Solve_SH23.py:409-545, FWD_Solve_KDyn.py:529-689,
 *                    FWD_Solve_IVP_Discrete FWD_Solve_SHB23.py:525-678          (returns the minimised value -J)
 *   smo_adjoint   <- ADJ_Solve_IVP_Lin      FWD_Solve_SH23.py:598-729 (+Compatib_Cond :552-596),
 *                                           FWD_Solve_KDyn.py:766-1004 (+Compatib_Cond :696-764),
 *                    ADJ_Solve_IVP_Discrete FWD_Solve_SHB23.py:796-920
 *   smo_inner     <- Inner_Prod             FWD_Solve_SH23.py:158-172, Inner_Prod_3 FWD_Solve_KDyn.py:173-181,
 *                    Inner_Prod_Discrete    FWD_Solve_SHB23.py:189-193
 *   SMO_POIS (stratified plane-Poiseuille optimal mixing, "Discrete" formulation): smo_forward <- FWD_Solve_Discrete
 *                    FWD_Solve_Poiseuille.py:777-1155, smo_adjoint <- ADJ_Solve_Discrete :1320-1659, smo_inner <- Inner_Prod_Discrete
 *                    :282-299, smo_transform <- transform / transformInverse / transformAdjoint / transformInverseAdjoint :44-89
 *
 * Conventions
 *   - every function returns SMO_OK (0) or an error code; smo_last_error() gives the message (thread local).
 *   - vectors are the reference's flat float64 grid vectors (Vec_to_Field / Field_to_Vec layouts):
 *       SH23 : 1 component, G = 2*npts values on the scale-2 Fourier grid
 *       SHB23: 1 component, npts values on the ascending Gauss-Chebyshev grid
 *       KDYN : 2 components (B0, U), each 3*G^3 (x,y,z parts concatenated, each C-ordered [x][y][z]), G = 3*npts/2
 *       POIS : 1 component [u.flatten(), w.flatten()] of the (Nx, Nz) grids, z fastest (Field_to_Vec, FWD_Solve_Poiseuille.py:160-207)
 *   - "_dev" entry points take pointers into the HBM of the context's device (no copies); the plain ones take
 *     caller-owned host buffers and stage them through context-owned device buffers.
 *   - all entry points are synchronous (return after the context's stream has drained).
 *   - smo_adjoint replays the snapshot stack filled by the last smo_forward of the same context and returns
 *     SMO_ERR_STATE if there was none (the reference's hidden contract).
 *   - `batch` > 1 runs that many independent problems per call (SH23, SHB23, KDYN on a plain single-GPU context: world == 1, not
 *     smo_create_multi; POIS in the Discrete formulation, cost 0 or 1): vectors are then [batch][len] per component (smo_vec_len stays per member; KDYN: X[c] = [batch][3 G^3] for B0 and
 *     U, host and _dev entry points alike), J / inner results are arrays of `batch` doubles, smo_adjoint fills every member's gradient and
 *     smo_snapshot_read reads member b.  KDYN: member b equals, bit for bit, a batch-1 solve of its inputs; smo_stack_bytes and the
 *     smo_timing_* byte figures count all members; ckpt applies one schedule to all members (0: the smallest interval whose `batch` stacks
 *     fit); smo_kdyn_op and smo_transform return SMO_ERR_UNSUPPORTED on a batched context.
 *     The members of a smo_create batch share smo_config.param; smo_create_members gives every member a value of its own (KDYN: Rm, SH23: a;
 *     SHB23 and POIS refuse it) and is otherwise the same batched context.  The members also share n_iters unless smo_set_horizons gives
 *     every member a horizon of its own (KDYN on one GPU, SH23); smo_config.n_iters is then the capacity.
 *     POIS: X[0] / grad[0] = [batch][2 Nx Nz]; the members share Re, Ri, Pr, delta and dt and therefore ONE set of tau operators, which a
 *     workgroup of the operator apply reads once for a group of 2 members by default (SMO_POIS_APPLY_MB = 1 | 2 | 4 forces the group size).
 *     Member b equals, bit for bit, a batch-1 solve of its input (J, gradient, <x,y>, every snapshot).  smo_stack_bytes = batch x the
 *     batch-1 figure; smo_config.ckpt applies one schedule to all members (a stack that does not fit: SMO_ERR_NOMEM at creation); the smo_timing_* byte figures are per launch of the whole
 *     batch; at most 1024 members (SMO_ERR_UNSUPPORTED beyond); smo_transform returns SMO_ERR_UNSUPPORTED on a batched context; the
 *     Continuous formulation (cost 2, 3) stays batch 1 (SMO_ERR_ARG), and so does the experimental SMO_POIS_XPROD=1.
 *   - one host thread per context; contexts are independent.
 *   - There is NO CPU fallback: without a usable HIP device smo_create fails with SMO_ERR_NO_DEVICE.
 */
#ifndef SMO_H_
#define SMO_H_

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct smo_ctx smo_ctx;

enum { SMO_OK = 0, SMO_ERR_ARG = 1, SMO_ERR_NO_DEVICE = 2, SMO_ERR_HIP = 3, SMO_ERR_STATE = 4, SMO_ERR_NOMEM = 5,
       SMO_ERR_UNSUPPORTED = 6 };

enum { SMO_SH23 = 1, SMO_SHB23 = 2, SMO_KDYN = 3, SMO_POIS = 4 }; /* smo_config.kind */
enum { SMO_POIS_KINETIC = 0, SMO_POIS_MIXNORM = 1,              /* smo_config.cost (POIS): the reference's switch s (FWD_Solve_Poiseuille.py:1761-1762), Discrete */
       SMO_POIS_CNTS_KINETIC = 2, SMO_POIS_CNTS_MIXNORM = 3 };   /* ... and the same two in the "Continuous" formulation (:614-775, :1161-1318) */
enum { SMO_COST_FINAL = 0, SMO_COST_INTEGRATED = 1 };           /* smo_config.cost (KDYN) */
enum { SMO_SHB_DISCRETE = 0, SMO_SHB_CONTINUOUS = 1 };          /* smo_config.cost (SHB23): formulation, FWD_Solve_SHB23.py:213-217 */
enum { SMO_ADJ_DISCRETE = 0, SMO_ADJ_CONTINUOUS = 1 };          /* `adjoint_type` argument */

typedef struct smo_config {
    int    kind;        /* SMO_SH23 | SMO_SHB23 | SMO_KDYN | SMO_POIS */
    int    npts;        /* Npts as the reference's Generate_IC receives it (SH23 256, SHB23 512, KDYN 128).  Like the reference, every kind takes the size it
                           is handed: SH23 ANY Npts >= 4; SHB23 ANY grid length in [4, 1024] (Continuous: Npts modes on the 2*Npts grid, Npts <= 512);
                           KDYN ANY even Npts >= 6 (FWD_Solve_SH23.py:279-332, FWD_Solve_SHB23.py:196-217, FWD_Solve_KDyn.py:362-450).  Tuned kernels
                           (compile-time transform lengths with factors 2, 3, 5, 7) exist for SH23 2^k, 3*2^k, 5*2^k, 7*2^k, 15*2^k in [16, 1024]; SHB23 2^k,
                           3*2^k in [64, 1024]; KDYN 8, 12, 16, 20, 24, 28, 32, 36, 40, 48, 56, 60, 64, 72, 80, 96, 100, 112, 120, 128, 144, 160, 192, 200,
                           224, 240, 256, 320.  Every other size (other prime factors, odd lengths) runs the same pipeline with the transform length a
                           run-time value (csrc/kdyn_any.hpp, sh23_*_any, the SHB23 kernels' NH = 0 form): 1.4-2.6x slower per grid point.  Outside these
                           ranges: SMO_ERR_UNSUPPORTED */
    double x0, x1;      /* interval of every axis: SH23 (0,12pi), SHB23 (-20,20), KDYN (0,2pi); only x1 - x0 enters (SHB23: the grid too).  KDYN
                           is built for a box of length 2 pi (integer wavenumbers): any other length is SMO_ERR_UNSUPPORTED */
    double dt;          /* time step */
    int    n_iters;     /* N_ITERS (the forward solve executes N_ITERS+1 steps for SH23/KDYN, like the reference) */
    double param;       /* SH23/SHB23: a (-0.3 / -0.1);  KDYN: Rm */
    int    cost;        /* KDYN: SMO_COST_FINAL | SMO_COST_INTEGRATED.  SHB23: SMO_SHB_DISCRETE (npts grid values = npts modes; snapshots
                           are grid states) | SMO_SHB_CONTINUOUS (npts modes, vectors hold the 2*npts values of the scale-2 grid,
                           snapshots are the npts T-coefficients; smo_adjoint must then be called with adjoint_type Continuous) */
    int    batch;       /* independent problems per call (>=1; KDYN: >1 only with world == 1, at most 65535; POIS: >1 only with cost 0 or 1, at most 1024) */
    int    device;      /* HIP device ordinal */
    /* slab decomposition of the 3-D case (one process per GPU; the exchange itself is done by the host layer):  */
    int    rank;        /* this process' slab index   (0 when world == 1) */
    int    world;       /* number of slabs            (1 = single GPU) */
    /* windowed checkpointing of the adjoint stack (KDYN on a single GPU; POIS, both formulations, any batch): keep every `ckpt`-th
     * snapshot and recompute the states in between, one window at a time, during the adjoint sweep (+ (ckpt-1)/ckpt forward steps per
     * adjoint step).  1 = keep everything (the reference's N_SUB_ITERS = N_ITERS); 0 = smallest interval whose stack fits the free HBM;
     * an interval beyond n_iters is one window (smo_get key 0 then reports n_iters).  The results are those of ckpt = 1 bit for bit.
     * POIS: with N = n_iters and k = ckpt > 1 the stack holds  N/k + 1 checkpoints (the states 0, k, 2k, ...)  +  1 slot for state N when
     * k does not divide N  +  min(k - 1, N - 1) window slots  <=  N/k + k + 1 records per member, a record being the snapshot
     * (smo_snapshot_len doubles) plus the 6 (Nx/2) tau scalars a restarted step reads beside it; smo_stack_bytes = slots x batch x record
     * (k = 1: N + 1 records of the snapshot alone).  smo_snapshot_read of a state that is not kept recomputes its window and returns the
     * keep-all bytes; smo_adjoint may follow.  ckpt = 0 counts the free HBM once every other buffer of the context is allocated, keeps
     * 1 GB spare, and fails with SMO_ERR_NOMEM when no interval fits; SMO_POIS_CKPT_BUDGET=<bytes> caps what it may assume free.
     * SMO_POIS_XPROD=1 (experimental) with an interval > 1: SMO_ERR_UNSUPPORTED. */
    int    ckpt;
    /* second resolution / further parameters (POIS only; zero elsewhere): npts = Nx and npts2 = Nz as the solver receives them (Discrete:
     * already scaled by 3/2, FWD_Solve_Poiseuille.py:1752-1755; Continuous: the mode counts, vectors then live on the 3/2 grid and
     * smo_adjoint must be called with adjoint_type Continuous); x0,x1 = the x interval (0, 4 pi), z is (-1, 1); param = Reynolds,
     * param2 = Richardson, param3 = Prandtl (0 -> 1), param4 = delta of the base density profile (0 -> 0.25); cost = s. */
    int    npts2;
    double param2, param3, param4;
} smo_config;

/* ---- life cycle ------------------------------------------------------------------------------------------- */
int         smo_create(const smo_config* cfg, smo_ctx** out);
/* ONE host process driving several GPUs of a node ("one host process driving the devices").  The reference's optimiser is a
 * single Python process; under `mpiexec -np P` every rank runs it redundantly and Dedalus moves the data (README.md:83, FWD_Solve_KDyn.py:118-134).
 * A multi-device context slab-decomposes a KDYN problem over `ndev` devices (cfg->rank / world stay 0 / 1, cfg->device is ignored; ndev must
 * divide npts/2 and 3*npts/2) behind the single-GPU calling sequence:
 *   smo_forward / smo_adjoint / smo_inner  take the reference's FULL flat host vectors [3][G][G][G] and return the full gradient: the library
 *       scatters / gathers the z slabs itself (the allgather of Field_to_Vec, FWD_Solve_KDyn.py:118-123, disappears);
 *   smo_forward_dev / smo_adjoint_dev      take ndev slab pointers per component instead: X[c * ndev + i] = component c's slab
 *       [3][G][G][G/ndev] in the HBM of dev_ids[i];
 * inside, one persistent worker thread per device runs the same in-library time loop as with one process per GPU, and a transpose is every
 * device pulling its blocks out of its peers' send buffers (peer access over xGMI), ordered by HIP events — ONE gather kernel per exchange that
 * reads all peers at once, or one hipMemcpyPeerAsync per peer (SMO_PEER_COPY=kernel|memcpy; smo_comm_get key 3 reports which is in use:
 * the kernel between ranks that share a device, the copy calls between distinct devices until the kernel has been verified on a multi-GPU
 * node) — no RCCL, no launcher, nothing for the caller to set up.  The same device may be listed more than once (tests on a one-GPU box).
 * Not available on such a context: smo_snapshot_read, smo_set_stream (SMO_ERR_UNSUPPORTED: every rank runs on a private stream of its own
 * device); smo_inner_dev is replaced by smo_inner_slabs; smo_timing_* report device 0's kernels.  smo_inner with full HOST vectors scatters
 * both vectors again on every call — an optimiser should keep its vectors distributed (one slab per device, smo_vec_*) and call
 * smo_inner_slabs (spheremanopt_amd/devvec.py: MultiDeviceVector). */
int         smo_create_multi(const smo_config* cfg, int ndev, const int* dev_ids, smo_ctx** out);
/* A batched context whose members each run with a parameter value of their own (a parameter study in one call): `params` is a host array of
 * cfg->batch doubles, member b runs with param = params[b] (KDYN: Rm, SH23: a) and cfg->param is ignored.  dt, n_iters, cost, ckpt and the
 * size stay shared, and everything a batched context of smo_create does or refuses holds unchanged (conventions above).  Member b equals, bit
 * for bit, a batch-1 smo_create context with param = params[b] on member b's input (J, gradients, <x,y>, every snapshot); all values equal:
 * the bits of the smo_create batch context with that param; batch == 1: exactly the smo_create context with param = params[0].
 *   SMO_SHB23, SMO_POIS: SMO_ERR_UNSUPPORTED (their parameter sits inside a tau operator: each member would need a tau operator of its own,
 *       where their batches are built on sharing one);
 *   params == NULL, a value that is not finite, KDYN: Rm <= 0, KDYN with world > 1 (batch 1 too): SMO_ERR_ARG, the message names the member.
 * There is no multi-device form.  The values are copied at creation (KDYN: into a device table the kernels read at their member index). */
int         smo_create_members(const smo_config* cfg, const double* params, smo_ctx** out);
/* A KDYN context whose velocity is FROZEN: the flow is given and only dJ/dB0 is asked for (optimal seed field, transient growth).  The G^
 * recursion of the adjoint reads U and the old G^ alone, so the context leaves out everything that serves dJ/dU: the adjoint x
 * pass forms omega x U only, no grid-side copy of the forward states is kept (smo_get key 1 reports 0), and dJ/dB0 is, bit for bit, that of the
 * smo_create / smo_create_members context of the same config.  cfg->kind must be SMO_KDYN and cfg->world 1 (anything else:
 * SMO_ERR_UNSUPPORTED; slabs and several devices are not built for this mode, and there is no smo_create_multi form); any batch.
 *   params      NULL: every member runs at cfg->param; else cfg->batch values of Rm with the contract and refusals of smo_create_members.
 *   keep_states 1: the snapshot stack and cfg->ckpt behave as in an ordinary context (keep-all, intervals, 0, dense tail, smo_snapshot_read with
 *                  window replay); with the Final cost the adjoint sweep reads B^_N alone and never replays a window.
 *               0: SMO_COST_FINAL only (Integrated reads every B^_n in its z update: SMO_ERR_ARG).  No stack: the forward solve alternates
 *                  between two slots, smo_stack_bytes = 2 x batch x snapshot bytes, cfg->ckpt is not consulted, smo_get key 0 reports n_iters,
 *                  smo_snapshot_read works for index n_iters and returns SMO_ERR_STATE for any other.
 * Calling sequence: smo_forward[_dev] takes X = {B0, U} as before (U may change between calls; smo_ncomp stays 2); smo_adjoint[_dev] fills
 * grad[0] only — grad[1] may be NULL and is never written; smo_inner*, smo_transform, smo_set_stream and the timing calls as on any single-GPU
 * KDYN context; smo_kdyn_op returns SMO_ERR_UNSUPPORTED. */
int         smo_create_frozen_u(const smo_config* cfg, const double* params, int keep_states, smo_ctx** out);
/* A time horizon of its own for every member (a growth curve — cost and optimal seed as functions of T — in one call).  cfg->n_iters stays the
 * CAPACITY: stack, partial sums and captured graphs are sized for it and smo_stack_bytes / smo_get key 0 do not change; member b then runs
 * n_iters[b] steps.  `n_iters`: cfg->batch values, each in [1, cfg->n_iters] (anything else: SMO_ERR_ARG, the message names the member); NULL: every
 * member back to cfg->n_iters.  smo_get_horizons fills cfg->batch values (cfg->n_iters each when none are set).
 *   Contexts: SMO_KDYN with world == 1 from smo_create, smo_create_members or smo_create_frozen_u (either keep_states), any batch including 1, and
 *       SMO_SH23.  SMO_SHB23, SMO_POIS, a KDYN slab context (world > 1) and a smo_create_multi context: SMO_ERR_UNSUPPORTED.
 *   Contract: member b's results are, bit for bit, those of a batch-1 context created with n_iters = n_iters[b] (and the member's own Rm / a) on
 *       member b's input — J, the gradients, both adjoint types, both costs, <x_b, y_b> and every snapshot, for every ckpt the context accepts.
 *       All values equal to cfg->n_iters, or none set: the bits of the context as it was.
 *   State: the call clears the forward state (smo_adjoint: SMO_ERR_STATE until the next smo_forward).  The values are copied into a device table;
 *       new values for an existing table keep the captured graphs of a KDYN context, the first table and its removal (NULL) drop them.
 *   smo_snapshot_read(ctx, b, i, ...) counts member b's own time: i in [0, n_iters[b]], beyond: SMO_ERR_ARG; a keep_states = 0 context holds
 *       i = n_iters[b] only.  smo_kdyn_op returns SMO_ERR_UNSUPPORTED while horizons are set.
 *   KDYN runs the members right-aligned in its n_iters-step launch sequence: member b idles through the first n_iters - n_iters[b] steps (its
 *       workgroups leave at entry) and runs its own last, so every member ends in the same snapshot.  The smo_timing_* byte
 *       figures stay per launch of the WHOLE batch: an upper bound once members idle. */
int         smo_set_horizons(smo_ctx* ctx, const int* n_iters);
int         smo_get_horizons(const smo_ctx* ctx, int* n_iters);
void        smo_destroy(smo_ctx* ctx);
const char* smo_last_error(void);
const char* smo_version(void);
int         smo_device_count(int* count);                      /* never initialises a device */
int         smo_device_cus(int device, int* cus);              /* compute units of a device (the grid unit of smo_lds_probe) */

/* ---- geometry --------------------------------------------------------------------------------------------- */
int smo_ncomp(const smo_ctx* ctx);                              /* number of norm-constrained vectors (1 or 2) */
int smo_vec_len(const smo_ctx* ctx, size_t* len);               /* doubles per component (per batch member) */
int smo_stack_bytes(const smo_ctx* ctx, size_t* bytes);         /* HBM held by the snapshot stack(s): checkpoints + window slots (smo_config.ckpt) */
/* key 0: checkpoint interval actually in use (1 = every snapshot kept; KDYN and POIS report what smo_config.ckpt = 0 chose);  key 1: KDYN: bytes of the y-side stack kept by the forward
 * solve so that the adjoint skips the z/y passes of every snapshot (0 if not in use); SHB23: how many calls fell back from the
 * multi-workgroup cluster to one workgroup per problem because a cluster all-gather timed out (a busy GPU);  key 2 (KDYN): number of
 * solves replayed from a captured HIP graph (small grids on one GPU: the whole forward solve / adjoint sweep is one graph launch); SHB23:
 * workgroups that co-operate on one problem (1 = no cluster: batch > 1, fewer than 256 modes, SMO_SHB_CLUSTER=0 or after a time-out);
 * key 3 (KDYN): layout of the y-transformed work fields, 0 = planes [c][kx][y][z], 1 = z-block major [c][z/8][kx][y][z%8];
 * key 4 (KDYN): milliseconds of HOST time the last smo_forward + smo_adjoint spent issuing work (entry of the call until everything is enqueued,
 * minus the waits for other ranks in host rendezvous; a multi-device context reports its slowest worker) — to be set against the kernels' time;
 * key 5 (KDYN): first snapshot index of the dense tail of the checkpoint schedule (every state from there on is kept), -1 = uniform interval;
 * key 6 (KDYN): 1 on a frozen-velocity context (smo_create_frozen_u), 0 otherwise;
 * key 7 (KDYN): the hand-over streams of the time loop this context stores write-through, one bit per stream (csrc/kdyn.hip, SMO_KD_WT; 0: none —
 * the build adopted none at this grid, the run-time-length kernels, or SMO_KD_WT=0 in the environment). */
int smo_get(const smo_ctx* ctx, int key, double* value);

/* ---- the three callbacks, host buffers ---------------------------------------------------------------------- */
int smo_forward(smo_ctx* ctx, const double* const* X, double* J);
int smo_adjoint(smo_ctx* ctx, const double* const* X, int adjoint_type, double* const* grad);
int smo_inner(smo_ctx* ctx, const double* x, const double* y, double* out);

/* ---- the three callbacks, device-resident buffers ------------------------------------------------------------ */
int smo_forward_dev(smo_ctx* ctx, const double* const* X_dev, double* J_host);
int smo_adjoint_dev(smo_ctx* ctx, const double* const* X_dev, int adjoint_type, double* const* grad_dev);
int smo_inner_dev(smo_ctx* ctx, const double* x_dev, const double* y_dev, double* out_host);
/* <x,y> of device-resident vectors given slab by slab: x_slabs[i] / y_slabs[i] = the slab in the HBM of the i-th device of a multi-device
 * context (smo_create_multi; the layout smo_forward_dev takes per component); a plain context has one slab, the vector itself. */
int smo_inner_slabs(smo_ctx* ctx, const double* const* x_slabs, const double* const* y_slabs, double* out_host);

/* ---- second order: Hessian-vector products (SMO_SH23) --------------------------------------------------------------------------------
 * H.V with H the Hessian of what smo_forward returned (f = -J), at the point X of the last smo_forward of the context: the EXACT derivative of
 * the Discrete gradient map X -> smo_adjoint(..., SMO_ADJ_DISCRETE, ...) in the direction V, symmetric in the context's inner product
 * (<W, H.V> = <V, H.W>) and linear in V (a power-of-two multiple of V gives that multiple of H.V bit for bit).  The Continuous adjoint is not
 * the gradient of anything discrete and has no such product.  Two sweeps per call: a tangent sweep forward in time, which reads the snapshot
 * stack and writes a second stack of the same shape, and a second-order adjoint sweep backward in time, which reads both.
 *   V / HV: lists of ONE vector each with the layout of X / grad, [batch][G] on the scale-2 grid; host buffers for smo_hessvec, pointers into the
 *       HBM of the context's device for smo_hessvec_dev.  dJ_host: `batch` HOST doubles, the directional derivatives <V_b, grad f_b> as the tangent
 *       sweep accumulates them; may be NULL.
 *   Contexts: SMO_SH23 from smo_create or smo_create_members, any batch, any Npts the context was created for, with or without
 *       smo_set_horizons: member b's H.V and dJ are, bit for bit, those of a batch-1 context created with the member's a and n_iters = n_iters[b].
 *       SMO_SHB23, SMO_KDYN, SMO_POIS and multi-device contexts: SMO_ERR_UNSUPPORTED.  An any-length context (no tuned instantiation, or
 *       SMO_SH_ANY=1) whose second-order sweep does not fit the LDS of a workgroup even as two rounds of two transforms (Npts beyond about 1270):
 *       SMO_ERR_UNSUPPORTED from this call — not from smo_create — with the byte counts in the message.
 *   SMO_ERR_ARG: a null list or vector, HV overlapping V (any overlap of the two [batch][G] ranges).
 *   State: needs the stack of a preceding smo_forward (SMO_ERR_STATE otherwise, and again after smo_set_horizons until the next smo_forward) and
 *       leaves the forward state alone: any number of directions may follow one smo_forward, and smo_adjoint stays valid before and after.
 *   Memory: the tangent stack (the bytes of the forward stack) comes from the context's pool at the FIRST call, not at creation; smo_stack_bytes
 *       counts it from then on (twice the figure at creation).  A context that never asks for a product allocates and reports as before.
 *   The two launches run on the context's stream and the call returns after it has drained, like smo_adjoint_dev.  Timing classes
 *       "sh23_tangent_kernel" and "sh23_soa_kernel", registered at the first call behind the classes the context had. */
int smo_hessvec(smo_ctx* ctx, const double* const* V, double* const* HV, double* dJ_host);
int smo_hessvec_dev(smo_ctx* ctx, const double* const* V_dev, double* const* HV_dev, double* dJ_host);

/* ---- across the members of a batched context: Gram matrix and recombination ------------------------------------------------------
 * Everything above treats the `batch` members as independent problems (smo_inner returns the batch values <x_b, y_b>).  These two are the
 * operations in which member a meets member b — what a block method needs (sub-optimal seeds, the singular spectrum of the propagator,
 * deflation, orthonormalisation, comparing two optima).  B = batch, len = smo_vec_len; x, y, out are ONE component's vectors [B][len]
 * (member stride len), host buffers for the plain forms, pointers into the HBM of the context's device for the _dev forms.
 *   smo_gram[_dev]     out[a*B + b] = (sum_k x_a[k] * y_b[k]) / scale — B*B HOST doubles, row-major; scale is the divisor of the context's own
 *       inner product (KDYN: G^3, SH23: G), applied as ONE rounded division of the finished sum, so out[b*B + b] is <x_b, y_b> of smo_inner up
 *       to rounding.  The k sum is taken in fixed-size pieces that are added in a fixed order: repeated calls return the same bits (no
 *       floating-point atomics), but NOT the bits of smo_inner, whose summation order differs.  y == x (the same pointer): the upper triangle is
 *       computed and mirrored, the result is exactly symmetric.
 *   smo_combine[_dev]  out_b[k] = sum_{a < B} C[a*B + b] * x_a[k], i.e. X.C with the members as columns; C: B*B HOST doubles, row-major,
 *       read during the call.  The sum over a is one chain of fused multiply-adds in ASCENDING a that starts from +0, the same for every k:
 *       a column of C whose only non-zero entry is s in row a gives out_b = fl(s * x_a) exactly (C = I copies, a permutation matrix permutes,
 *       diag(s) is smo_vec_axpby(s_b, x_b); a -0 comes out as +0).
 *   Both are dense products: a non-finite value propagates into every entry it takes part in (0 * NaN is NaN, also under a zero of C).
 *   Contexts: SMO_KDYN with world == 1 on one device (smo_create, smo_create_members, smo_create_frozen_u with either keep_states, with or
 *       without horizons) and SMO_SH23, batch 1 .. 256 (batch 1: <x, y> and a scaled copy).  SMO_ERR_UNSUPPORTED: SMO_SHB23 and SMO_POIS (their
 *       inner products carry weights), slab and multi-device contexts, batch > 256.
 *   SMO_ERR_ARG: a null pointer, a pointer that is not 8-byte aligned, `out` overlapping `x` in smo_combine* (any overlap of the two B*len
 *       ranges: every output member reads every input member).
 *   The work runs on the context's stream and the call returns after it has drained, like smo_inner_dev.  The forward state is not touched:
 *       smo_adjoint after smo_forward stays valid with these calls in between.  Each x (and y) element is read from HBM once per call up to 64
 *       members; beyond, the members are worked in blocks of 64 x 64.  Timing classes "block_gram(x,x)", "block_gram(x,y)", "block_combine". */
int smo_gram(smo_ctx* ctx, const double* x, const double* y, double* out);
int smo_gram_dev(smo_ctx* ctx, const double* x_dev, const double* y_dev, double* out_host);
int smo_combine(smo_ctx* ctx, const double* C, const double* x, double* out);
int smo_combine_dev(smo_ctx* ctx, const double* C_host, const double* x_dev, double* out_dev);
/* FOR TESTS ONLY, and free to change with the kernels' tuning (do not build on the values): how smo_gram* cuts the element axis on this
 * context, so that a test can aim at the seams: geo[0] = elements per chunk, geo[1] = chunks per
 * workgroup (workgroup g owns the elements [g*geo[0]*geo[1], (g+1)*geo[0]*geo[1])), geo[2] = workgroups (= partial sums per entry),
 * geo[3] = elements per workgroup of smo_combine*.  Same refusals as smo_gram. */
int smo_gram_geometry(smo_ctx* ctx, size_t* geo);

/* ---- device-resident vectors for the caller's own vector algebra ------------------------------------------------
 * The reference's optimiser does X + alpha*d, coeff*X, -1.*g + beta*t and deepcopy on full-size NumPy vectors
 * (Sphere_Grad_Descent.py:284, 296-298, 625-690, 755-756, 813) and the callbacks then move them over PCIe on every call.  With
 * these entry points the vectors stay in HBM (spheremanopt_amd/devvec.py wraps them in a class with +, -, scalar *, deepcopy) and
 * go to smo_forward_dev / smo_adjoint_dev / smo_inner_dev as they are.
 *   - buffers come from a per-device pool (smo_vec_free returns them to it; smo_vec_pool_release gives the memory back);
 *   - smo_vec_axpby: out[i] = fl( fl(a*x[i]) + fl(b*y[i]) ), y == NULL: out[i] = fl(a*x[i]); products and sum are rounded
 *     separately (no fused multiply-add), i.e. bit for bit what NumPy computes for a*x + b*y; out may alias x or y;
 *   - all of them are synchronous — and they run on a stream of the pool's own: the operands must be COMPLETE when the call is made
 *     (results of smo_*_dev calls are: those return after their stream has drained; work a caller has enqueued itself on another
 *     stream, e.g. the one handed to smo_set_stream, must be synchronised first);
 *   - smo_vec_axpby takes any 8-byte-aligned device pointers (pool buffers are 256-byte aligned and use 16-byte accesses; a view at an
 *     odd element offset of a caller's own buffer runs the same arithmetic one element per lane); anything else: SMO_ERR_ARG. */
int smo_vec_alloc(int device, size_t n, double** out_dev);
int smo_vec_free(int device, double* dev);
int smo_vec_pool_release(int device);
int smo_vec_pool_bytes(int device, size_t* live, size_t* pooled);
int smo_vec_upload(int device, double* dev, const double* host, size_t n);
int smo_vec_download(int device, const double* dev, double* host, size_t n);
int smo_vec_axpby(int device, size_t n, double a, const double* x_dev, double b, const double* y_dev, double* out_dev);
/* page-locked host memory for the host-buffer entry points (smo_forward / smo_adjoint / smo_inner copy at PCIe rate from / to it;
 * from pageable memory the runtime stages through its own bounce buffers) */
int smo_host_alloc(size_t bytes, void** out);
int smo_host_free(void* p);

/* Guard zones (test instrumentation, the counterpart for writes of the SMO_POISON fill).  With SMO_GUARD=<cap in bytes> in the environment
 * — read at each allocation; a whole number, a multiple of 256 in 4096 .. 2^30, anything else is SMO_ERR_ARG at the allocation — every
 * device block the library allocates (every buffer of every context, every device vector; not the pinned host blocks) is laid out as
 *     [front zone][block][slack up to the next multiple of 256][back zone],   each zone clamp(round_up(requested bytes, 256), 4096, cap)
 * bytes of a position-dependent pattern that is written on the device before the block is handed out.  The pointer handed out keeps its
 * 256-byte alignment; smo_stack_bytes, smo_vec_pool_bytes and every checkpoint choice count the same bytes as without the knob.  Zones and
 * slack of a block are compared on the device when the block is given back (smo_destroy, smo_vec_free, buffers a context replaces), after
 * the device has drained; whether a block is guarded is kept with the block.  Unset: one getenv per allocation and today's layout.
 * smo_guard_report: if ctx is non-null, drains it and checks every live block of its pool (a multi-device context: of every rank's pool)
 * now; in every case checks the live and pooled device vectors of all devices; adds what the frees recorded since the last report; returns
 * the number of blocks checked and of blocks found damaged, and in first[0 .. first_len) the description of the first damaged block —
 * allocation site, requested bytes, zone ("front zone", "slack", "back zone"), the first damaged byte as "start-<k>" (k bytes before the
 * block) or "end+<k>" (k bytes past the requested bytes), and the number of damaged 8-byte words — or "".  Any pointer may be null.  The
 * tally is reset, and a block found damaged is patterned again: a second report counts only what was stored after the first.  With the
 * knob never set it reports 0 / 0. */
int smo_guard_report(smo_ctx* ctx, size_t* checked, size_t* damaged, char* first, size_t first_len);

/* LDS fill (test instrumentation, the sibling of SMO_POISON for the LDS).  With SMO_POISON_LDS=<0..255> in the environment — read where a
 * context is created and where the device-vector entry points are entered (and by smo_lds_probe), never at a launch; the value of the last
 * read holds process-wide until the next one; anything but a whole number in 0..255 is SMO_ERR_ARG at those places — every kernel launch of
 * the library is preceded on its stream (inside a stream capture: as a node of the same graph, so a replay fills again) by a fill dispatch
 * that leaves that byte in every byte of every CU's LDS.  Results must be bit for bit those of the run without the knob.  Unset: one
 * test of a cached value per launch.
 * smo_lds_probe: reads the knob, then launches through the same hook, on `device`, `workgroups` workgroups (at most 65536) of 256 threads
 * with `lds_bytes` (a multiple of 8, at most the device's LDS per workgroup) of dynamic LDS each; a workgroup reads its own LDS without
 * writing it and counts the 8-byte words whose every byte is the knob's byte (knob unset: 0).  *words = workgroups * lds_bytes / 8,
 * *words_equal_fill = the count.  With lds_bytes = 0 or workgroups = 0 nothing is launched.  In every case *fills_launched = the fill
 * dispatches issued and *launches_hooked = the launches that found the knob set, both process-wide since the last call (the probe's own
 * launch included), and both are reset; equal counts mean that no launch went without its fill, 0 / 0 that the knob was unset throughout.
 * Any pointer may be null.  The probe waits for its own launch only and sees only the CUs its workgroups land on: a grid of at least the
 * CU count, of workgroups that take the whole LDS, reaches every CU. */
int smo_lds_probe(int device, size_t lds_bytes, size_t workgroups, size_t* words, size_t* words_equal_fill, size_t* fills_launched,
                  size_t* launches_hooked);

/* ---- introspection used by the parity tests and the benchmark ------------------------------------------------ */
/* Copy snapshot `index` (0..n_iters) of batch member `b` to the host in the reference's GEN_BUFFER element order:
 * SH23 complex128[Nc]; SHB23 float64[N]; KDYN complex128[3][a][m][m]; POIS complex128[3][Nx/2][Nz] (u_fwd, w_fwd, b_fwd of the
 * non-negative wavenumbers).  `out` receives smo_snapshot_len doubles.  After smo_set_horizons `index` counts member b's own time,
 * 0..n_iters[b]. */
int smo_snapshot_len(const smo_ctx* ctx, size_t* ndoubles);
int smo_snapshot_read(smo_ctx* ctx, int b, int index, double* out);

/* The reference's standalone transforms, host buffers: which = 0 transform (grid -> coefficients), 1 transformInverse,
 * 2 transformAdjoint (coefficients -> grid), 3 transformInverseAdjoint (grid -> coefficients).
 *   SHB23 (FWD_Solve_SHB23.py:36-67): npts doubles either way.
 *   POIS  (FWD_Solve_Poiseuille.py:44-89): grid = float64[Nx][Nz] of a REAL field, coefficients = complex128[a][Nz] for the
 *          non-negative x wavenumbers n = 0..a-1, a = Nx/2 (the other half of the reference's complex spectrum is the Hermitian mirror). */
/*   KDYN  (the transforms Dedalus performs for field['c'] / field['g'], FWD_Solve_KDyn.py:139-171, 635-637): which = 0: three grid fields
 *          float64[3][G][G][G] -> truncated coefficients complex128[3][a][m][m]; which = 1: the inverse (zero padding, c2r ignores Im of kx = 0). */
int smo_transform(smo_ctx* ctx, int which, const double* in, double* out);

/* ---- slab-decomposed 3-D case: one process per GPU ---------------------------------
 * With smo_config.world > 1 a KDYN context owns the kx-slab [rank*a/world, (rank+1)*a/world) of every coefficient
 * field and the z-slab of every grid field; vectors are then the LOCAL slabs [3][G][G][G/world].  The pencil transpose sits
 * between the z and the y pass, where a field is smallest (16*a*m*G bytes per component), as one all-to-all per direction per
 * step carrying every field of that direction.
 *
 * (1) In-library time loop — what the reference gets from Dedalus' in-library MPI transposes (FWD_Solve_KDyn.py:118-134,
 *     README.md:83 `mpiexec -np 4`): give the context a communicator ONCE, then smo_forward[_dev] / smo_adjoint[_dev] /
 *     smo_inner[_dev] are called collectively by all ranks exactly like their single-GPU forms (J and <x,y> come back reduced).
 *       smo_comm_unique_id   rank 0: 128 opaque bytes (an RCCL unique id) to hand to every rank by any means (MPI, a file,
 *                            torch.distributed, ...);
 *       smo_comm_init        collective: ncclCommInitRank over smo_config.world ranks; the transposes are then grouped
 *                            ncclSend/ncclRecv on HIP streams of the solver (chunk-pipelined with the grid-side kernels), the scalar
 *                            reductions ncclAllReduce;
 *       smo_comm_set_transport  instead of RCCL: caller-provided all-to-all / all-reduce (tests in which ranks share a GPU or run over
 *                            gloo); collective as well.
 *     Both agree, across the ranks, on the checkpoint interval and on whether the grid-side states are kept (every rank takes those
 *     decisions from its own free HBM) before the first exchange could mismatch.
 * (2) Phase-level entry (smo_kdyn_op): the same loop cut into the phases between two exchanges, for a host layer that performs
 *     the transposes itself (spheremanopt_amd/kdyn_slab.py: torch.distributed; kept as the CPU/gloo test harness). */
typedef int (*smo_alltoall_fn)(void* user, const void* src_dev, void* dst_dev, size_t bytes_per_peer, void* hip_stream);
typedef int (*smo_allreduce_fn)(void* user, double* host_values, int n);      /* in place: sum over the ranks */
int smo_comm_unique_id(void* id128);
int smo_comm_init(smo_ctx* ctx, const void* id128);
int smo_comm_set_transport(smo_ctx* ctx, smo_alltoall_fn all_to_all, smo_allreduce_fn all_reduce_sum, void* user);
/* (all three arguments NULL: the null transport — exchanges and reductions do nothing.  For profiling one rank's share of a W-way decomposition
 * on a single GPU through the real in-library loop, tools/prof_slab_geometry.py; the results of such a solve are meaningless.) */
/* key 0: pipelined z chunks per exchange; 1: field-group exchanges per forward+adjoint step pair; 2: 1 if the transport is RCCL;
 * multi-device contexts: 3: how a transpose pulls (2 = gather kernel, 1 = hipMemcpyPeerAsync calls), 4: host rendezvous passed so far */
int smo_comm_get(const smo_ctx* ctx, int key, double* value);
/* File of the librccl this library bound for smo_comm_unique_id / smo_comm_init (dladdr of its ncclGetUniqueId), "" if none can be
 * loaded.  A copy already in the process (PyTorch bundles one) is reused, else the system library is loaded; the environment variable
 * SMO_RCCL_LIB (a path or soname) replaces that search.  What the reference gets from `mpiexec` picking ONE MPI library for every rank
 * (README.md:83): a process holding two RCCL copies would otherwise not know which one carries the transposes. */
const char* smo_comm_library(void);
/* If smo_comm_init / smo_comm_set_transport fail after the transport exists (the ranks chose different checkpoint intervals from their
 * free HBM, ...), the transport is dropped again: the context is back in its "no communicator" state (smo_forward: SMO_ERR_STATE)
 * and the call may be repeated. */

/* The exchange buffers hold [chunk][peer][field group][3][a/world][m][G/world/chunks] complex128; peer blocks are contiguous.
 *   z-side buffer: my kx, peer = z block; written by the inverse z pass, read by the forward z pass
 *   y-side buffer: peer = kx block, my z; read by the inverse y pass, written by the forward y pass
 * Phases only enqueue work on the context's stream (see smo_set_stream); SMO_KD_ENERGY / SMO_KD_SYNC synchronise. */
enum {
    SMO_KD_SET_BUFFERS = 0,   /* p0 = z-side, p1 = y-side exchange buffer, each 2*elems complex128 (elems: SMO_KD_EXCHANGE_ELEMS);
                                 layout [peer][field group][3][a/W][m][G/W]: z side = my kx, peer's z block; y side = peer's kx, my z  */
    SMO_KD_EXCHANGE_ELEMS = 1,/* out <- complex128 elements of ONE field group summed over all peers (= 3*(a/W)*m*G)                */
    SMO_KD_G2C_A = 2,         /* p0 = local grid vector [3][G][G][G/W]: x, y passes grid -> spectrum           [then exchange y->z] */
    SMO_KD_G2C_C = 3,         /* z pass + truncation; i0 = 0: store as snapshot 0 (B0), 1: store as scratch (U^)                     */
    SMO_KD_C2G_A = 4,         /* i0 = 0: dt*alpha*G^ (discrete grad B), 1: G^/scratch, 2: nu^ ; z pass         [then exchange z->y] */
    SMO_KD_C2G_B = 5,         /* y, x passes spectrum -> grid; p0 = output local grid vector, NULL = the context's U field           */
    SMO_KD_FWD_A = 6,         /* i0 = step n: z inverse pass of snapshot n                                  [exchange z->y, 1 group] */
    SMO_KD_FWD_B = 7,         /* i0 = n: y pass, fused x pass (c2r, U x B, r2c), y pass                     [exchange y->z, 1 group] */
    SMO_KD_FWD_C = 8,         /* i0 = n: z forward pass + curl, projection, CNAB1 update -> snapshot n+1                             */
    SMO_KD_ENERGY = 9,        /* i0 = n: out <- this slab's share of <B_n,B_n> (synchronises)                                        */
    SMO_KD_ADJ_INIT = 10,     /* i0 = adjoint_type: terminal condition from snapshot N                                               */
    SMO_KD_ADJ_A = 11,        /* i0 = snapshot index: z inverse pass of curl(G^) [and of B^_i0]       [exchange z->y, 1 or 2 groups:
                                 1 when smo_get(ctx, 1) > 0 (grid-side states kept by the forward solve) and i0 < n_iters, else 2]   */
    SMO_KD_ADJ_B = 12,        /* i0 = snapshot index: y pass(es), fused x pass (two cross products; the second one, (curl G) x B_i0, is
                                 added to a running sum that stays on the grid side), y pass of the first [exchange y->z, 1 group]    */
    SMO_KD_ADJ_C = 13,        /* i0 = snapshot index: z forward pass + G^ update                                                     */
    SMO_KD_SYNC = 14,         /* wait for the context's stream                                                                     */
    SMO_KD_SET_CHUNKS = 15,   /* i0 = K: cut the local z slab into K equal chunks.  The grid-side phases (G2C_A, C2G_B, FWD_B, ADJ_B, NU_B) then
                                 take the chunk index in i1 and the exchange buffers become [chunk][peer][field group][3][a/W][m][G/W/K]:
                                 every chunk is one contiguous all-to-all, so the host layer can overlap the exchange of one chunk with
                                 the grid work on another.  K = 1 (default) is the layout described above.                            */
    SMO_KD_NU_B = 16,         /* after the last adjoint step; i1 = chunk: y pass of the running sum                 [exchange y->z, 1 group] */
    SMO_KD_NU_C = 17          /* z forward pass of it, projection, factor -dt  ->  nu^ (= the reference's nu recursion: it acts as the
                                 identity on the solenoidal sums it carries, so the transforms are applied once instead of per step)   */
};
int smo_kdyn_op(smo_ctx* ctx, int op, int i0, int i1, void* p0, void* p1, double* out);

/* Enqueue all further work of the context on a caller-owned HIP stream (e.g. torch.cuda.current_stream().cuda_stream) so
 * that collectives issued by the host layer on that stream are ordered with the kernels without host synchronisation.
 * SMO_ERR_UNSUPPORTED on a multi-device context (smo_create_multi). */
int smo_set_stream(smo_ctx* ctx, void* hip_stream);

/* HIP-event timing of the kernels launched by the context (measured on the context's stream).
 * smo_timing_enable(ctx, on) resets the accumulators; on = 0 off, 1 every class, 2 + k only class k, k < 64 (two event records per
 * launch cost ~2 us on the GPU, so the benchmark times only the dominant class inside its timed region); smo_timing_get returns, for kernel class `k`
 * (0 <= k < smo_timing_classes), its name, number of launches, total milliseconds and the ALGORITHMIC bytes
 * one launch moves (DESIGN.md section "kernels"), so  achieved GB/s = bytes * launches / ms / 1e6.  The byte figures are per launch of the
 * whole batch: with smo_set_horizons in force the members that idle through a launch move nothing, and the figures are an upper bound. */
int         smo_timing_enable(smo_ctx* ctx, int on);
/* time exactly the classes whose bit is set in `class_mask` (bit k = class k; 0 = off); resets the accumulators.  The multi-GPU benchmark
 * times its dominant kernel class AND the "slab_exchange(all-to-all)" class (events around every grouped send/recv, on the stream it runs on). */
int         smo_timing_select(smo_ctx* ctx, unsigned long long class_mask);
/* of the selected classes, time every `every`-th launch only (default 1 = all): the averages become those of a uniform sample of the launches,
 * the event records (two per timed launch, each a marker in the queue that keeps the next kernel from overlapping the previous one's tail)
 * cost 1/every as much.  Stays in force until changed; smo_timing_get's `launches` counts the TIMED launches. */
int         smo_timing_stride(smo_ctx* ctx, int every);
int         smo_timing_classes(const smo_ctx* ctx);
int         smo_timing_get(smo_ctx* ctx, int k, const char** name, long long* launches, double* total_ms,
                           double* bytes_per_launch);
/* Compulsory HBM bytes of one launch of class `k` AS FUSED (every input read once, every output written once) —
 * the denominator of the roofline fraction.  The algorithmic figure of smo_timing_get also prices the axis passes the fusion removed
 * and is therefore >= this one. */
int         smo_timing_hbm_bytes(smo_ctx* ctx, int k, double* bytes_per_launch);

#ifdef __cplusplus
}
#endif
#endif /* SMO_H_ */
