// jacprod.cpp -- the Jacobian-product handle of libopty_hip.so: J(free) v and
// J(free)^T w without the matrix (include/opty_hip.h, "matrix-free Jacobian
// products").
//
// The handle borrows its problem handle (device, stream, known parameters,
// known trajectories, h, instance atom indices): one copy of the known data,
// and what opty_hip_set_known_* installs is what the next product reads.  The
// generated code object exports `opty_jvp` (lane = constraint node, grid.y =
// strips of the equations), `opty_jvp_inst` (one lane, the instance
// constraints' rows), `opty_vjp` (lane = constraint node, blocks that overlap
// by one node, grid.y = strips of the free rows; one partial per block and
// tail column) and `opty_vjp_fin` (one wave: the partials' sums, then the
// instance constraints' contributions).
#include "opty_internal.h"

using namespace opty;

namespace {

// The packed kernarg buffer of the four kernels; must match JACPROD_PARAMS in
// opty_amd/codegen/emit_jacprod.py.
struct JacprodArgs {
    const double *free_;
    const double *known_traj;
    const double *params;
    const double *vec;
    const long long *inst_idx;
    double *out;
    double *part;
    double h;
    long long N;
};
static_assert(sizeof(JacprodArgs) == 72,
              "JacprodArgs must match JACPROD_PARAMS");

// constraint nodes a block of opty_vjp advances by (VJP_STRIDE of
// emit_jacprod.py): 64 lanes, the first repeats the previous block's last
constexpr long long kVjpStride = 63;

}  // namespace

struct opty_hip_jacprod : Borrowed {
    opty_hip_jacprod_desc d{};
    hipFunction_t k_jvp = nullptr, k_jvp_inst = nullptr, k_vjp = nullptr,
                  k_vjp_fin = nullptr;
    double *d_part = nullptr;   // num_tail partials per block of opty_vjp
    // staging for host callers
    double *d_free = nullptr, *d_vec = nullptr, *d_out = nullptr;
    long long ncn() const { return p->d.N - 1; }
    long long vjp_blocks() const {
        return (ncn() + kVjpStride - 1)/kVjpStride;
    }
};

namespace {

// One product: `nvec` doubles of `vec` in, `nout` doubles out.
template <typename Launch>
int run(opty_hip_jacprod *h, const double *free_, const double *vec,
        size_t nvec, double *out, size_t nout, int32_t mem, Launch launch) {
    if (!h || !free_ || !vec || !out) return fail("null argument");
    if (int rc = borrowed_begin(h, mem, true)) return rc;
    opty_hip_problem *p = h->p;
    const size_t nfree = (size_t)p->num_free();
    JacprodArgs a{};
    a.vec = vec;
    a.out = out;
    a.part = h->d_part;
    if (mem == OPTY_HIP_HOST) {
        // one staging vector each, sized for either product
        const size_t big = std::max<size_t>(
            1, std::max(nfree, (size_t)p->num_con()));
        if (int rc = stage_in(h, &free_, &h->d_free, nfree, nfree)) return rc;
        if (int rc = stage_in(h, &a.vec, &h->d_vec, nvec, big)) return rc;
        if (int rc = ensure(&h->d_out, big)) return rc;
        a.out = h->d_out;
    }
    borrowed_args(&a, p, free_);
    size_t size = sizeof a;
    void *config[] = {HIP_LAUNCH_PARAM_BUFFER_POINTER, &a,
                      HIP_LAUNCH_PARAM_BUFFER_SIZE, &size,
                      HIP_LAUNCH_PARAM_END};
    if (int rc = launch(config)) return rc;
    if (mem == OPTY_HIP_HOST) {
        if (int rc = stage_out(h, out, h->d_out, nout*sizeof(double)))
            return rc;
        return host_done(h);
    }
    return 0;
}

}  // namespace

extern "C" {

int opty_hip_jacprod_create(opty_hip_problem *p,
                            const opty_hip_jacprod_desc *desc,
                            const char *code_object_path,
                            opty_hip_jacprod **out) {
    if (!p || !desc || !code_object_path || !out)
        return fail("null argument");
    if (desc->jvp_strips < 1 || desc->vjp_strips < 1 || desc->num_tail < 0 ||
        desc->nnz_inst < 0)
        return fail("bad Jacobian-product descriptor (jvp_strips %d, "
                    "vjp_strips %d, num_tail %d, nnz_inst %d)",
                    desc->jvp_strips, desc->vjp_strips, desc->num_tail,
                    desc->nnz_inst);
    if (desc->num_tail != p->d.r + p->d.s)
        return fail("num_tail %d, but the problem has %d unknown parameters "
                    "and %d free intervals", desc->num_tail, p->d.r, p->d.s);
    if (desc->nnz_inst > 0 && p->d.num_inst == 0)
        return fail("instance entries but the problem has no instance "
                    "constraints");
    if (p->d.N < 2) return fail("N %lld < 2", (long long)p->d.N);
    if (int rc = use_device(p)) return rc;
    auto *h = new opty_hip_jacprod;
    h->d = *desc;
    if (int rc = borrowed_create(h, p, code_object_path,
                                 {{&h->k_jvp, "opty_jvp", true},
                                  {&h->k_jvp_inst, "opty_jvp_inst", true},
                                  {&h->k_vjp, "opty_vjp", true},
                                  {&h->k_vjp_fin, "opty_vjp_fin", true}},
                                 nullptr)) {
        delete h;
        return rc;
    }
    if (desc->num_tail > 0) {
        // one partial per block of opty_vjp and tail column
        hipError_t m = hipMalloc(
            (void **)&h->d_part,
            (size_t)desc->num_tail*(size_t)h->vjp_blocks()*sizeof(double));
        if (m != hipSuccess) {
            (void)hipGetLastError();
            (void)opty_hip_jacprod_destroy(h);
            return fail("hipMalloc of the partials failed: %s",
                        hipGetErrorString(m));
        }
    }
    *out = h;
    return 0;
}

int opty_hip_jacprod_destroy(opty_hip_jacprod *h) {
    if (!h) return 0;
    borrowed_destroy(h, {h->d_part, h->d_free, h->d_vec, h->d_out});
    delete h;
    return 0;
}

int opty_hip_jacprod_jvp(opty_hip_jacprod *h, const double *free_,
                         const double *v, double *out, int32_t mem) {
    if (!h) return fail("null argument");
    opty_hip_problem *p = h->p;
    const long long nblk = (h->ncn() + 63)/64;
    return run(h, free_, v, (size_t)p->num_free(), out, (size_t)p->num_con(),
               mem, [&](void **config) -> int {
        if (p->d.M > 0)
            HIP_TRY(hipModuleLaunchKernel(h->k_jvp, (unsigned)nblk,
                                          (unsigned)h->d.jvp_strips, 1, 64, 1,
                                          1, 0, h->stream, nullptr, config));
        if (p->d.num_inst > 0)
            HIP_TRY(hipModuleLaunchKernel(h->k_jvp_inst, 1, 1, 1, 64, 1, 1, 0,
                                          h->stream, nullptr, config));
        return 0;
    });
}

int opty_hip_jacprod_vjp(opty_hip_jacprod *h, const double *free_,
                         const double *w, double *out, int32_t mem) {
    if (!h) return fail("null argument");
    opty_hip_problem *p = h->p;
    return run(h, free_, w, (size_t)p->num_con(), out, (size_t)p->num_free(),
               mem, [&](void **config) -> int {
        HIP_TRY(hipModuleLaunchKernel(h->k_vjp, (unsigned)h->vjp_blocks(),
                                      (unsigned)h->d.vjp_strips, 1, 64, 1, 1,
                                      0, h->stream, nullptr, config));
        if (h->d.num_tail > 0 || h->d.nnz_inst > 0)
            HIP_TRY(hipModuleLaunchKernel(h->k_vjp_fin, 1, 1, 1, 64, 1, 1, 0,
                                          h->stream, nullptr, config));
        return 0;
    });
}

}  // extern "C"
