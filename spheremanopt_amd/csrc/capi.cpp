// extern "C" surface of libsmo (declarations and reference citations: include/smo.h).
#include "smo_common.hpp"
#include "blockops_tiles.hpp"
#include "comm.hpp"

#include <cmath>

using smo::Context;

struct smo_ctx {
    Context* impl;
};

#define CHECK_CTX(c)                                  \
    do {                                              \
        if (!(c) || !(c)->impl) {                     \
            smo::set_error("null context");           \
            return SMO_ERR_ARG;                       \
        }                                             \
    } while (0)

extern "C" {

const char* smo_last_error(void) { return smo::last_error(); }
const char* smo_version(void) { return "libsmo 0.1.0 (gfx950)"; }

int smo_device_count(int* count) {
    if (!count) return SMO_ERR_ARG;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    *count = (e == hipSuccess) ? n : 0;
    return SMO_OK;
}

int smo_device_cus(int device, int* cus) {
    if (!cus) return SMO_ERR_ARG;
    *cus = 0;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { smo::set_error("no usable HIP device; libsmo has no CPU fallback"); return SMO_ERR_NO_DEVICE; }
    if (device < 0 || device >= ndev) { smo::set_error("device %d out of range (have %d)", device, ndev); return SMO_ERR_ARG; }
    SMO_HIP(hipDeviceGetAttribute(cus, hipDeviceAttributeMultiprocessorCount, device));
    return SMO_OK;
}

// The KDyn kernels carry the integer wavenumbers of a 2 pi box: another box length would be solved as if it were 2 pi.
static int check_kdyn_interval(const smo_config* cfg, const char* who) {
    const double two_pi = 6.283185307179586476925286766559;
    if (cfg->kind != SMO_KDYN || std::fabs((cfg->x1 - cfg->x0) - two_pi) <= 1e-9 * two_pi) return SMO_OK;
    smo::set_error("%s: KDYN is built for a box of length 2 pi on every axis; interval [%.17g, %.17g] has length %.17g", who, cfg->x0,
                   cfg->x1, cfg->x1 - cfg->x0);
    return SMO_ERR_UNSUPPORTED;
}

// `params`: one value per member (smo_create_members), null for smo_create; frozen_u / keep_states: smo_create_frozen_u
static int create_single(const smo_config* cfg, const double* params, const char* who, smo_ctx** out, bool frozen_u = false, bool keep_states = true) {
    if (cfg->batch < 1 || cfg->n_iters < 1 || cfg->npts < 4 || !(cfg->dt > 0) || !(cfg->x1 > cfg->x0) || cfg->world < 1 ||
        cfg->rank < 0 || cfg->rank >= cfg->world || cfg->ckpt < 0) {
        smo::set_error("%s: bad config (npts=%d n_iters=%d dt=%g batch=%d interval=[%g,%g] rank=%d/%d)", who, cfg->npts,
                       cfg->n_iters, cfg->dt, cfg->batch, cfg->x0, cfg->x1, cfg->rank, cfg->world);
        return SMO_ERR_ARG;
    }
    SMO_TRY(check_kdyn_interval(cfg, who));
    Context* c = nullptr;
    switch (cfg->kind) {
        case SMO_SH23: c = smo::make_sh23(*cfg); break;
        case SMO_SHB23: c = smo::make_shb23(*cfg); break;
        case SMO_KDYN: c = smo::make_kdyn(*cfg); break;
        case SMO_POIS: c = smo::make_pois(*cfg); break;
        default: smo::set_error("%s: unknown kind %d", who, cfg->kind); return SMO_ERR_ARG;
    }
    if (!c) return SMO_ERR_UNSUPPORTED;      // message set by the factory
    if (params) c->member_params.assign(params, params + cfg->batch);
    c->frozen_u = frozen_u; c->keep_states = keep_states;
    int rc = c->init();
    if (rc == SMO_OK) rc = c->block_register();      // timing classes of smo_gram* / smo_combine*, behind the context's own
    if (rc != SMO_OK) { delete c; return rc; }
    *out = new smo_ctx{c};
    return SMO_OK;
}

int smo_create(const smo_config* cfg, smo_ctx** out) {
    if (!cfg || !out) { smo::set_error("smo_create: null argument"); return SMO_ERR_ARG; }
    *out = nullptr;
    return create_single(cfg, nullptr, "smo_create", out);
}

int smo_create_members(const smo_config* cfg, const double* params, smo_ctx** out) {
    if (!cfg || !out) { smo::set_error("smo_create_members: null argument"); return SMO_ERR_ARG; }
    *out = nullptr;
    if (cfg->kind == SMO_SHB23 || cfg->kind == SMO_POIS) {
        smo::set_error("smo_create_members: %s keeps its parameter inside a tau operator, so each member would need a tau operator of its own; "
                       "its batches share one (KDYN and SH23 take one value per member)", cfg->kind == SMO_SHB23 ? "SHB23" : "POIS");
        return SMO_ERR_UNSUPPORTED;
    }
    if (cfg->kind != SMO_KDYN && cfg->kind != SMO_SH23) { smo::set_error("smo_create_members: unknown kind %d", cfg->kind); return SMO_ERR_ARG; }
    if (cfg->batch < 1) { smo::set_error("smo_create_members: batch = %d", cfg->batch); return SMO_ERR_ARG; }
    if (!params) { smo::set_error("smo_create_members: params is null (one value for each of the %d members, member 0 first)", cfg->batch); return SMO_ERR_ARG; }
    for (int b = 0; b < cfg->batch; ++b) {
        if (!std::isfinite(params[b])) { smo::set_error("smo_create_members: member %d: the value is not finite (%g)", b, params[b]); return SMO_ERR_ARG; }
        if (cfg->kind == SMO_KDYN && !(params[b] > 0)) { smo::set_error("smo_create_members: member %d: Rm = %g (KDYN: Rm > 0)", b, params[b]); return SMO_ERR_ARG; }
    }
    if (cfg->kind == SMO_KDYN && cfg->world != 1) {
        smo::set_error("smo_create_members: KDYN members (member 0 .. %d) with their own Rm run on one GPU (world = 1, got %d)", cfg->batch - 1, cfg->world);
        return SMO_ERR_ARG;
    }
    smo_config c = *cfg;
    c.param = params[0];                      // cfg->param is ignored
    // one member: exactly the smo_create context of that value
    return create_single(&c, c.batch == 1 ? nullptr : params, "smo_create_members", out);
}

// one Rm per member: every value finite and > 0 (the message names the member)
static int check_member_rm(const smo_config* cfg, const double* params, const char* who) {
    for (int b = 0; b < cfg->batch; ++b) {
        if (!std::isfinite(params[b])) { smo::set_error("%s: member %d: the value is not finite (%g)", who, b, params[b]); return SMO_ERR_ARG; }
        if (!(params[b] > 0)) { smo::set_error("%s: member %d: Rm = %g (KDYN: Rm > 0)", who, b, params[b]); return SMO_ERR_ARG; }
    }
    return SMO_OK;
}

int smo_create_frozen_u(const smo_config* cfg, const double* params, int keep_states, smo_ctx** out) {
    if (!cfg || !out) { smo::set_error("smo_create_frozen_u: null argument"); return SMO_ERR_ARG; }
    *out = nullptr;
    if (cfg->kind != SMO_KDYN) {
        smo::set_error("smo_create_frozen_u: kind %d — only KDYN has a second vector (the velocity) to freeze", cfg->kind);
        return SMO_ERR_UNSUPPORTED;
    }
    if (cfg->world != 1) {
        smo::set_error("smo_create_frozen_u: a frozen-velocity context runs on one GPU (world = 1, got %d); slabs and multi-device are not built", cfg->world);
        return SMO_ERR_UNSUPPORTED;
    }
    if (keep_states != 0 && keep_states != 1) { smo::set_error("smo_create_frozen_u: keep_states = %d (0 or 1)", keep_states); return SMO_ERR_ARG; }
    if (!keep_states && cfg->cost != SMO_COST_FINAL) {
        smo::set_error("smo_create_frozen_u: keep_states = 0 with the Integrated cost — its adjoint reads every forward state B^_n in the z update, "
                       "so the states must be kept (keep_states = 1); only the Final cost reads B^_N alone");
        return SMO_ERR_ARG;
    }
    if (cfg->batch < 1) { smo::set_error("smo_create_frozen_u: batch = %d", cfg->batch); return SMO_ERR_ARG; }
    smo_config c = *cfg;
    if (params) {
        SMO_TRY(check_member_rm(cfg, params, "smo_create_frozen_u"));
        c.param = params[0];                  // cfg->param is ignored
    }
    // one member: the context of that value, no table (as smo_create_members)
    return create_single(&c, (params && c.batch > 1) ? params : nullptr, "smo_create_frozen_u", out, true, keep_states != 0);
}

int smo_create_multi(const smo_config* cfg, int ndev, const int* dev_ids, smo_ctx** out) {
    if (!cfg || !out || !dev_ids) { smo::set_error("smo_create_multi: null argument"); return SMO_ERR_ARG; }
    *out = nullptr;
    if (cfg->batch != 1 || cfg->n_iters < 1 || cfg->npts < 4 || !(cfg->dt > 0) || !(cfg->x1 > cfg->x0) || cfg->ckpt < 0 || ndev < 1 || ndev > 64) {
        smo::set_error("smo_create_multi: bad config (npts=%d n_iters=%d dt=%g batch=%d ndev=%d)", cfg->npts, cfg->n_iters, cfg->dt, cfg->batch, ndev);
        return SMO_ERR_ARG;
    }
    SMO_TRY(check_kdyn_interval(cfg, "smo_create_multi"));
    Context* c = smo::make_multi(*cfg, ndev, dev_ids);
    int rc = c->init();
    if (rc != SMO_OK) { delete c; return rc; }
    *out = new smo_ctx{c};
    return SMO_OK;
}

void smo_destroy(smo_ctx* ctx) {
    if (!ctx) return;
    if (ctx->impl) {
        (void)hipSetDevice(ctx->impl->cfg.device);
        delete ctx->impl;
    }
    delete ctx;
}

// SMO_GUARD: the zones of the context's live blocks and of every device vector now, plus what the frees recorded since the last report
int smo_guard_report(smo_ctx* ctx, size_t* checked, size_t* damaged, char* first, size_t first_len) {
    if (ctx && !ctx->impl) { smo::set_error("null context"); return SMO_ERR_ARG; }
    int rc = SMO_OK;
    if (ctx) {
        SMO_HIP(hipSetDevice(ctx->impl->cfg.device));
        rc = ctx->impl->guard_check_live();
    }
    if (rc == SMO_OK) rc = smo::vec_guard_check_all();
    smo::guard_take(checked, damaged, first, first_len);
    return rc;
}

int smo_ncomp(const smo_ctx* ctx) { return (ctx && ctx->impl) ? ctx->impl->n_comp : 0; }

int smo_vec_len(const smo_ctx* ctx, size_t* len) {
    CHECK_CTX(ctx);
    if (!len) return SMO_ERR_ARG;
    *len = ctx->impl->vec_len;
    return SMO_OK;
}
int smo_stack_bytes(const smo_ctx* ctx, size_t* bytes) {
    CHECK_CTX(ctx);
    if (!bytes) return SMO_ERR_ARG;
    *bytes = ctx->impl->stack_bytes;
    return SMO_OK;
}

int smo_get(const smo_ctx* ctx, int key, double* value) {
    CHECK_CTX(ctx);
    if (!value || key < 0 || key > 7) { smo::set_error("smo_get: bad argument"); return SMO_ERR_ARG; }
    *value = ctx->impl->info(key);
    return SMO_OK;
}

// `dev`: the list holds device pointers (a multi-device context then dereferences one slab per component AND device: every one is checked)
static int check_vecs(const smo_ctx* ctx, const double* const* X, const char* who, bool dev = false) {
    if (!X) { smo::set_error("%s: null vector list", who); return SMO_ERR_ARG; }
    const int n = dev ? ctx->impl->n_dev_ptrs() : ctx->impl->n_comp;
    for (int c = 0; c < n; ++c)
        if (!X[c]) { smo::set_error("%s: pointer %d of %d is null", who, c, n); return SMO_ERR_ARG; }
    return SMO_OK;
}

int smo_forward(smo_ctx* ctx, const double* const* X, double* J) {
    CHECK_CTX(ctx);
    SMO_TRY(check_vecs(ctx, X, "smo_forward"));
    if (!J) return SMO_ERR_ARG;
    return ctx->impl->forward_host(X, J);
}
int smo_forward_dev(smo_ctx* ctx, const double* const* X, double* J) {
    CHECK_CTX(ctx);
    SMO_TRY(check_vecs(ctx, X, "smo_forward_dev", true));
    if (!J) return SMO_ERR_ARG;
    SMO_HIP(hipSetDevice(ctx->impl->cfg.device));
    return ctx->impl->forward_dev(X, J);
}

static int check_adjoint(smo_ctx* ctx, int adjoint_type, double* const* grad, bool dev = false) {
    if (adjoint_type != SMO_ADJ_DISCRETE && adjoint_type != SMO_ADJ_CONTINUOUS) {
        smo::set_error("smo_adjoint: adjoint_type %d", adjoint_type);
        return SMO_ERR_ARG;
    }
    if (!ctx->impl->have_forward) {
        smo::set_error("smo_adjoint: no forward solve on this context yet (the adjoint replays its snapshot stack)");
        return SMO_ERR_STATE;
    }
    if (ctx->impl->n_grads() == ctx->impl->n_comp) return check_vecs(ctx, grad, "smo_adjoint(grad)", dev);
    // a frozen-velocity context fills grad[0] alone: grad[1] may be null and is never written
    if (!grad || !grad[0]) { smo::set_error("smo_adjoint(grad): null vector list or null grad[0]"); return SMO_ERR_ARG; }
    return SMO_OK;
}
int smo_adjoint(smo_ctx* ctx, const double* const* X, int adjoint_type, double* const* grad) {
    CHECK_CTX(ctx);
    SMO_TRY(check_adjoint(ctx, adjoint_type, grad));
    return ctx->impl->adjoint_host(X, adjoint_type, grad);
}
int smo_adjoint_dev(smo_ctx* ctx, const double* const* X, int adjoint_type, double* const* grad) {
    CHECK_CTX(ctx);
    SMO_TRY(check_adjoint(ctx, adjoint_type, grad, true));
    SMO_HIP(hipSetDevice(ctx->impl->cfg.device));
    return ctx->impl->adjoint_dev(X, adjoint_type, grad);
}

// kind, pointers, overlap, state — all before anything is allocated or launched
static int check_hessvec(smo_ctx* ctx, const double* const* V, double* const* HV, const char* who) {
    Context* c = ctx->impl;
    SMO_TRY(c->check_hessvec());
    if (!V || !HV || !V[0] || !HV[0]) { smo::set_error("%s: null vector (V and HV are lists of one vector [batch][G] each)", who); return SMO_ERR_ARG; }
    const size_t bytes = c->vec_len * (size_t)c->cfg.batch * sizeof(double);
    const char *v = reinterpret_cast<const char*>(V[0]), *h = reinterpret_cast<const char*>(HV[0]);
    if (v < h + bytes && h < v + bytes) { smo::set_error("%s: HV overlaps V (the direction is read while the product is written)", who); return SMO_ERR_ARG; }
    if (!c->have_forward) {
        smo::set_error("%s: no forward solve on this context yet (the tangent sweep reads its snapshot stack)", who);
        return SMO_ERR_STATE;
    }
    return SMO_OK;
}
int smo_hessvec(smo_ctx* ctx, const double* const* V, double* const* HV, double* dJ_host) {
    CHECK_CTX(ctx);
    SMO_TRY(check_hessvec(ctx, V, HV, "smo_hessvec"));
    return ctx->impl->hessvec_host(V, HV, dJ_host);
}
int smo_hessvec_dev(smo_ctx* ctx, const double* const* V_dev, double* const* HV_dev, double* dJ_host) {
    CHECK_CTX(ctx);
    SMO_TRY(check_hessvec(ctx, V_dev, HV_dev, "smo_hessvec_dev"));
    SMO_HIP(hipSetDevice(ctx->impl->cfg.device));
    return ctx->impl->hessvec_dev(V_dev, HV_dev, dJ_host);
}

int smo_inner(smo_ctx* ctx, const double* x, const double* y, double* out) {
    CHECK_CTX(ctx);
    if (!x || !y || !out) { smo::set_error("smo_inner: null argument"); return SMO_ERR_ARG; }
    return ctx->impl->inner_host(x, y, out);
}
int smo_inner_dev(smo_ctx* ctx, const double* x, const double* y, double* out) {
    CHECK_CTX(ctx);
    if (!x || !y || !out) { smo::set_error("smo_inner_dev: null argument"); return SMO_ERR_ARG; }
    SMO_HIP(hipSetDevice(ctx->impl->cfg.device));
    return ctx->impl->inner_dev(x, y, out);
}

int smo_inner_slabs(smo_ctx* ctx, const double* const* x, const double* const* y, double* out) {
    CHECK_CTX(ctx);
    if (!x || !y || !out) { smo::set_error("smo_inner_slabs: null argument"); return SMO_ERR_ARG; }
    for (int i = 0; i < ctx->impl->n_slabs(); ++i)
        if (!x[i] || !y[i]) { smo::set_error("smo_inner_slabs: slab %d of %d is null", i, ctx->impl->n_slabs()); return SMO_ERR_ARG; }
    SMO_HIP(hipSetDevice(ctx->impl->cfg.device));
    return ctx->impl->inner_slabs(x, y, out);
}

// Gram matrix and recombination across the members of a batched context (csrc/blockops.hip); the context checks kind, batch, alignment, overlap
int smo_gram(smo_ctx* ctx, const double* x, const double* y, double* out) {
    CHECK_CTX(ctx);
    if (!x || !y || !out) { smo::set_error("smo_gram: null argument"); return SMO_ERR_ARG; }
    SMO_HIP(hipSetDevice(ctx->impl->cfg.device));
    return ctx->impl->gram_host(x, y, out);
}
int smo_gram_dev(smo_ctx* ctx, const double* x, const double* y, double* out) {
    CHECK_CTX(ctx);
    if (!x || !y || !out) { smo::set_error("smo_gram_dev: null argument"); return SMO_ERR_ARG; }
    SMO_HIP(hipSetDevice(ctx->impl->cfg.device));
    return ctx->impl->gram_dev(x, y, out);
}
int smo_combine(smo_ctx* ctx, const double* C, const double* x, double* out) {
    CHECK_CTX(ctx);
    if (!C || !x || !out) { smo::set_error("smo_combine: null argument"); return SMO_ERR_ARG; }
    SMO_HIP(hipSetDevice(ctx->impl->cfg.device));
    return ctx->impl->combine_host(C, x, out);
}
int smo_combine_dev(smo_ctx* ctx, const double* C, const double* x, double* out) {
    CHECK_CTX(ctx);
    if (!C || !x || !out) { smo::set_error("smo_combine_dev: null argument"); return SMO_ERR_ARG; }
    SMO_HIP(hipSetDevice(ctx->impl->cfg.device));
    return ctx->impl->combine_dev(C, x, out);
}

int smo_gram_geometry(smo_ctx* ctx, size_t* geo) {
    CHECK_CTX(ctx);
    if (!geo) { smo::set_error("smo_gram_geometry: null argument"); return SMO_ERR_ARG; }
    SMO_TRY(ctx->impl->block_check("smo_gram_geometry"));
    const smo::blockops::GramPlan p = smo::blockops::gram_plan(ctx->impl->cfg.batch, ctx->impl->vec_len);
    geo[0] = (size_t)p.kc; geo[1] = p.cpw; geo[2] = (size_t)p.nwg; geo[3] = (size_t)smo::blockops::kThreads;
    return SMO_OK;
}

int smo_snapshot_len(const smo_ctx* ctx, size_t* n) {
    CHECK_CTX(ctx);
    if (!n) return SMO_ERR_ARG;
    *n = ctx->impl->snapshot_doubles;
    return SMO_OK;
}
int smo_set_horizons(smo_ctx* ctx, const int* n_iters) {
    CHECK_CTX(ctx);
    Context* c = ctx->impl;
    SMO_TRY(c->check_horizons());
    for (int b = 0; n_iters && b < c->cfg.batch; ++b)
        if (n_iters[b] < 1 || n_iters[b] > c->cfg.n_iters) {
            smo::set_error("smo_set_horizons: member %d: %d steps (1 .. %d, the n_iters the context was created with)", b, n_iters[b], c->cfg.n_iters);
            return SMO_ERR_ARG;
        }
    SMO_HIP(hipSetDevice(c->cfg.device));
    return c->set_horizons(n_iters);
}
int smo_get_horizons(const smo_ctx* ctx, int* n_iters) {
    CHECK_CTX(ctx);
    if (!n_iters) { smo::set_error("smo_get_horizons: null argument"); return SMO_ERR_ARG; }
    const Context* c = ctx->impl;
    for (int b = 0; b < c->cfg.batch; ++b) n_iters[b] = c->horizons.empty() ? c->cfg.n_iters : c->horizons[b];
    return SMO_OK;
}

int smo_snapshot_read(smo_ctx* ctx, int b, int index, double* out) {
    CHECK_CTX(ctx);
    // (a member with its own horizon: the index counts its own time, 0 .. N_b)
    if (!out || b < 0 || b >= ctx->impl->cfg.batch || index < 0 || index > (ctx->impl->horizons.empty() ? ctx->impl->cfg.n_iters : ctx->impl->horizons[b])) {
        smo::set_error("smo_snapshot_read: bad argument (b=%d index=%d)", b, index);
        return SMO_ERR_ARG;
    }
    if (!ctx->impl->have_forward) { smo::set_error("smo_snapshot_read: no forward solve yet"); return SMO_ERR_STATE; }
    SMO_HIP(hipSetDevice(ctx->impl->cfg.device));
    return ctx->impl->snapshot_read(b, index, out);
}

int smo_transform(smo_ctx* ctx, int which, const double* in, double* out) {
    CHECK_CTX(ctx);
    if (!in || !out || which < 0 || which > 3) { smo::set_error("smo_transform: bad argument"); return SMO_ERR_ARG; }
    SMO_HIP(hipSetDevice(ctx->impl->cfg.device));
    return ctx->impl->transform_host(which, in, out);
}

int smo_kdyn_op(smo_ctx* ctx, int op, int i0, int i1, void* p0, void* p1, double* out) {
    CHECK_CTX(ctx);
    SMO_HIP(hipSetDevice(ctx->impl->cfg.device));
    return ctx->impl->kdyn_op(op, i0, i1, p0, p1, out);
}

int smo_comm_unique_id(void* id128) {
    if (!id128) { smo::set_error("smo_comm_unique_id: null argument"); return SMO_ERR_ARG; }
    return smo::SlabComm::unique_id(id128);
}
int smo_comm_init(smo_ctx* ctx, const void* id128) {
    CHECK_CTX(ctx);
    if (!id128) { smo::set_error("smo_comm_init: null id"); return SMO_ERR_ARG; }
    SMO_HIP(hipSetDevice(ctx->impl->cfg.device));
    return ctx->impl->comm_init(id128);
}
int smo_comm_set_transport(smo_ctx* ctx, smo_alltoall_fn a2a, smo_allreduce_fn ared, void* user) {
    CHECK_CTX(ctx);
    SMO_HIP(hipSetDevice(ctx->impl->cfg.device));
    return ctx->impl->comm_set_transport(a2a, ared, user);
}
const char* smo_comm_library(void) { return smo::SlabComm::library_path(); }
int smo_comm_get(const smo_ctx* ctx, int key, double* value) {
    CHECK_CTX(ctx);
    if (!value || key < 0 || key > 4) { smo::set_error("smo_comm_get: bad argument"); return SMO_ERR_ARG; }
    *value = ctx->impl->comm_info(key);
    return SMO_OK;
}

int smo_set_stream(smo_ctx* ctx, void* hip_stream) {
    CHECK_CTX(ctx);
    SMO_HIP(hipSetDevice(ctx->impl->cfg.device));
    return ctx->impl->set_stream(static_cast<hipStream_t>(hip_stream));
}

int smo_timing_enable(smo_ctx* ctx, int on) {
    CHECK_CTX(ctx);
    if (on < 0 || on - 2 >= 64) { smo::set_error("smo_timing_enable: on = %d (0, 1, or 2 + class index < 64)", on); return SMO_ERR_ARG; }
    ctx->impl->tm().reset();
    ctx->impl->tm().on = (on != 0);
    ctx->impl->tm().mask = (on >= 2) ? (1ull << (on - 2)) : ~0ull;
    return SMO_OK;
}
int smo_timing_select(smo_ctx* ctx, unsigned long long class_mask) {
    CHECK_CTX(ctx);
    ctx->impl->tm().reset();
    ctx->impl->tm().on = (class_mask != 0);
    ctx->impl->tm().mask = class_mask;
    return SMO_OK;
}
int smo_timing_stride(smo_ctx* ctx, int every) {
    CHECK_CTX(ctx);
    if (every < 1) { smo::set_error("smo_timing_stride: every = %d (>= 1 expected)", every); return SMO_ERR_ARG; }
    ctx->impl->tm().stride = every;
    return SMO_OK;
}
int smo_timing_classes(const smo_ctx* ctx) { return (ctx && ctx->impl) ? (int)ctx->impl->tm().cls.size() : 0; }
int smo_timing_get(smo_ctx* ctx, int k, const char** name, long long* launches, double* total_ms, double* bytes_per_launch) {
    CHECK_CTX(ctx);
    auto& t = ctx->impl->tm();
    if (k < 0 || k >= (int)t.cls.size()) { smo::set_error("smo_timing_get: class %d", k); return SMO_ERR_ARG; }
    (void)ctx->impl->sync_all();
    t.flush();
    if (name) *name = t.cls[k].name.c_str();
    if (launches) *launches = t.cls[k].launches;
    if (total_ms) *total_ms = t.cls[k].total_ms;
    if (bytes_per_launch) *bytes_per_launch = t.cls[k].bytes_per_launch;
    return SMO_OK;
}
int smo_timing_hbm_bytes(smo_ctx* ctx, int k, double* bytes_per_launch) {
    CHECK_CTX(ctx);
    auto& t = ctx->impl->tm();
    if (k < 0 || k >= (int)t.cls.size() || !bytes_per_launch) { smo::set_error("smo_timing_hbm_bytes: class %d", k); return SMO_ERR_ARG; }
    *bytes_per_launch = t.cls[k].hbm_bytes;
    return SMO_OK;
}

}  // extern "C"
