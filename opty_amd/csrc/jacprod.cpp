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
//
// Block products (opty_hip_jacprod_block_*): a handle of its own over a module
// of its own -- `opty_jvp_block`, `opty_jvp_block_inst`, `opty_vjp_block`,
// `opty_vjp_block_fin`, the four kernels above for `width` columns per pass.
#include "opty_internal.h"

#include <algorithm>
#include <cstddef>
#include <vector>

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
    long long wa, wb;      // the window of constraint nodes
    long long ostride;     // row stride of `out`; its first column is node wa
    double *tail;          // opty_jvp_inst: the o instance rows;
                           // opty_vjp_fin: the r + s tail sums
};
static_assert(sizeof(JacprodArgs) == 104,
              "JacprodArgs must match JACPROD_PARAMS");

// ... and of the four block kernels (JACPROD_BLOCK_PARAMS)
struct JacprodBlockArgs {
    const double *free_;
    const double *known_traj;
    const double *params;
    const double *vec;
    const long long *inst_idx;
    double *out;
    double *part;
    double h;
    long long N;
    long long ldv, ldo;
    int ncols;
};
static_assert(offsetof(JacprodBlockArgs, ncols) == 88,
              "JacprodBlockArgs must match JACPROD_BLOCK_PARAMS");

// constraint nodes a block of opty_vjp advances by (VJP_STRIDE of
// emit_jacprod.py): 64 lanes, the first repeats the previous block's last
constexpr long long kVjpStride = 63;

}  // namespace

struct opty_hip_jacprod : Borrowed {
    opty_hip_jacprod_desc d{};
    hipFunction_t k_jvp = nullptr, k_jvp_inst = nullptr, k_vjp = nullptr,
                  k_vjp_fin = nullptr;
    double *d_part = nullptr;   // num_tail partials per block of opty_vjp
    std::vector<double> zero_tail;  // what an empty window's tail sums are
    // staging for host callers
    double *d_free = nullptr, *d_vec = nullptr, *d_out = nullptr;
    long long ncn() const { return p->d.N - 1; }
    // blocks of opty_vjp for the window [wa, wb) (vjp_window_blocks of
    // emit_jacprod.py; opty_vjp_fin computes the same): the first block of a
    // window that starts at node 0 writes 64 entries, every other block 63
    long long vjp_blocks(long long wa, long long wb) const {
        const long long pend = wb + (wb == ncn() ? 1 : 0);
        const long long span = pend - wa - (wa == 0 ? 1 : 0);
        return span > 0 ? (span + kVjpStride - 1)/kVjpStride : 1;
    }
    // ... for the largest window, the whole problem
    long long vjp_blocks() const { return vjp_blocks(0, ncn()); }
};

struct opty_hip_jacprod_block : Borrowed {
    opty_hip_jacprod_block_desc d{};
    hipFunction_t k_jvp = nullptr, k_jvp_inst = nullptr, k_vjp = nullptr,
                  k_vjp_fin = nullptr;
    double *d_part = nullptr;   // num_tail*width partials per block
    // staging for host callers: `free`, and the columns of both blocks
    // without their padding (grown to the widest call so far)
    double *d_free = nullptr, *d_vec = nullptr, *d_out = nullptr;
    size_t cap_vec = 0, cap_out = 0;
    long long ncn() const { return p->d.N - 1; }
    long long vjp_blocks() const {
        return (ncn() + kVjpStride - 1)/kVjpStride;
    }
};

namespace {

int grow(double **ptr, size_t *cap, size_t count) {
    if (*ptr && *cap >= count) return 0;
    if (*ptr) {
        HIP_TRY(hipFree(*ptr));
        *ptr = nullptr;
        *cap = 0;
    }
    if (int rc = ensure(ptr, count)) return rc;
    *cap = count;
    return 0;
}

bool meets(const double *a, size_t na, const double *b, size_t nb) {
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a0 < b0 + nb*sizeof(double) && b0 < a0 + na*sizeof(double);
}

// One block product: `ncols` columns of `nvec` doubles in (`vname`, leading
// dimension `ldv`), as many of `nout` doubles out (`oname`, `ldo`);
// `launch(config, width)` enqueues one pass.
template <typename Launch>
int run_block(opty_hip_jacprod_block *h, const double *free_,
              const double *vec, const char *vname, int64_t ldv, size_t nvec,
              double *out, const char *oname, int64_t ldo, size_t nout,
              int32_t ncols, int32_t mem, Launch launch) {
    if (!h || !free_ || !vec || !out) return fail("null argument");
    if (ncols < 0) return fail("ncols %d < 0", ncols);
    if (ldv < (int64_t)nvec)
        return fail("ld%s %lld < column length %zu", vname, (long long)ldv,
                    nvec);
    if (ldo < (int64_t)nout)
        return fail("ld%s %lld < column length %zu", oname, (long long)ldo,
                    nout);
    opty_hip_problem *p = h->p;
    const size_t nfree = (size_t)p->num_free();
    if (ncols > 0) {
        const size_t no = (size_t)(ncols - 1)*(size_t)ldo + nout,
                     nv = (size_t)(ncols - 1)*(size_t)ldv + nvec;
        if (meets(out, no, vec, nv))
            return fail("%s (%d columns, ld %lld) overlaps %s (ld %lld)",
                        oname, ncols, (long long)ldo, vname, (long long)ldv);
        if (meets(out, no, free_, nfree))
            return fail("%s (%d columns, ld %lld) overlaps the %zu values of "
                        "free", oname, ncols, (long long)ldo, nfree);
    }
    if (int rc = borrowed_begin(h, mem, true)) return rc;
    if (ncols == 0) return 0;
    const double *dvec = vec;
    double *dout = out;
    long long dldv = ldv, dldo = ldo;
    if (mem == OPTY_HIP_HOST) {
        // the columns without their padding
        if (int rc = stage_in(h, &free_, &h->d_free, nfree, nfree)) return rc;
        if (int rc = grow(&h->d_vec, &h->cap_vec, (size_t)ncols*nvec))
            return rc;
        if (int rc = grow(&h->d_out, &h->cap_out, (size_t)ncols*nout))
            return rc;
        for (int c = 0; c < ncols && nvec; ++c)
            HIP_TRY(hipMemcpyAsync(h->d_vec + (size_t)c*nvec,
                                   vec + (size_t)c*(size_t)ldv,
                                   nvec*sizeof(double),
                                   hipMemcpyHostToDevice, h->stream));
        dvec = h->d_vec;
        dout = h->d_out;
        dldv = (long long)nvec;
        dldo = (long long)nout;
    }
    // ceil(ncols / width) passes; the last one as wide as what is left
    for (int c = 0; c < ncols; c += h->d.width) {
        JacprodBlockArgs a{};
        borrowed_args(&a, p, free_);
        a.vec = dvec + (size_t)c*(size_t)dldv;
        a.out = dout + (size_t)c*(size_t)dldo;
        a.part = h->d_part;
        a.ldv = dldv;
        a.ldo = dldo;
        a.ncols = std::min(h->d.width, ncols - c);
        size_t size = offsetof(JacprodBlockArgs, ncols) + sizeof a.ncols;
        void *config[] = {HIP_LAUNCH_PARAM_BUFFER_POINTER, &a,
                          HIP_LAUNCH_PARAM_BUFFER_SIZE, &size,
                          HIP_LAUNCH_PARAM_END};
        if (int rc = launch(config)) return rc;
    }
    if (mem == OPTY_HIP_HOST) {
        for (int c = 0; c < ncols; ++c)
            if (int rc = stage_out(h, out + (size_t)c*(size_t)ldo,
                                   h->d_out + (size_t)c*nout,
                                   nout*sizeof(double)))
                return rc;
        return host_done(h);
    }
    return 0;
}

// One product of the whole problem (`jvp`, or vjp): `nvec` doubles of `vec`
// in, `nout` doubles out.
template <typename Launch>
int run(opty_hip_jacprod *h, bool jvp, const double *free_, const double *vec,
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
    // the whole problem: every constraint node, the vector's own strides,
    // the instance rows / tail sums where the vector has them
    a.wa = 0;
    a.wb = h->ncn();
    a.ostride = jvp ? h->ncn() : (long long)p->d.N;
    a.tail = a.out + (jvp ? (size_t)p->d.M*(size_t)h->ncn()
                          : nfree - (size_t)h->d.num_tail);
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

// The window check the *_shard entry points share.
int check_window(const opty_hip_jacprod *h, int64_t a, int64_t b) {
    if (a < 0 || b > (int64_t)h->ncn() || a > b)
        return fail("node window [%lld, %lld) is not within the %lld "
                    "constraint nodes", (long long)a, (long long)b,
                    h->ncn());
    return 0;
}

// One windowed launch sequence on the problem's stream, device pointers only.
template <typename Launch>
int run_window(opty_hip_jacprod *h, const double *free_, const double *vec,
               double *out, int64_t out_stride, double *tail, int64_t wa,
               int64_t wb, Launch launch) {
    if (int rc = borrowed_begin(h, OPTY_HIP_DEVICE, true)) return rc;
    JacprodArgs a{};
    borrowed_args(&a, h->p, free_);
    a.vec = vec;
    a.out = out;
    a.part = h->d_part;
    a.wa = wa;
    a.wb = wb;
    a.ostride = out_stride;
    a.tail = tail;
    size_t size = sizeof a;
    void *config[] = {HIP_LAUNCH_PARAM_BUFFER_POINTER, &a,
                      HIP_LAUNCH_PARAM_BUFFER_SIZE, &size,
                      HIP_LAUNCH_PARAM_END};
    return launch(config);
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
    return run(h, true, free_, v, (size_t)p->num_free(), out,
               (size_t)p->num_con(), mem, [&](void **config) -> int {
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
    return run(h, false, free_, w, (size_t)p->num_con(), out,
               (size_t)p->num_free(), mem, [&](void **config) -> int {
        HIP_TRY(hipModuleLaunchKernel(h->k_vjp, (unsigned)h->vjp_blocks(),
                                      (unsigned)h->d.vjp_strips, 1, 64, 1, 1,
                                      0, h->stream, nullptr, config));
        if (h->d.num_tail > 0 || h->d.nnz_inst > 0)
            HIP_TRY(hipModuleLaunchKernel(h->k_vjp_fin, 1, 1, 1, 64, 1, 1, 0,
                                          h->stream, nullptr, config));
        return 0;
    });
}

int opty_hip_jacprod_jvp_shard(opty_hip_jacprod *h, const double *free_,
                               const double *v, double *out,
                               int64_t out_stride, int64_t node_begin,
                               int64_t node_end) {
    if (!h || !free_ || !v || !out) return fail("null argument");
    if (int rc = check_window(h, node_begin, node_end)) return rc;
    if (out_stride < node_end - node_begin)
        return fail("out_stride %lld < the %lld nodes of the window",
                    (long long)out_stride,
                    (long long)(node_end - node_begin));
    if (node_begin == node_end || h->p->d.M == 0) return 0;
    const long long nblk = (node_end - node_begin + 63)/64;
    return run_window(h, free_, v, out, out_stride, nullptr, node_begin,
                      node_end, [&](void **config) -> int {
        HIP_TRY(hipModuleLaunchKernel(h->k_jvp, (unsigned)nblk,
                                      (unsigned)h->d.jvp_strips, 1, 64, 1, 1,
                                      0, h->stream, nullptr, config));
        return 0;
    });
}

int opty_hip_jacprod_jvp_instance(opty_hip_jacprod *h, const double *free_,
                                  const double *v, double *out_tail) {
    if (!h || !free_ || !v) return fail("null argument");
    if (h->p->d.num_inst == 0) return 0;
    if (!out_tail) return fail("null argument");
    return run_window(h, free_, v, nullptr, 0, out_tail, 0, 0,
                      [&](void **config) -> int {
        HIP_TRY(hipModuleLaunchKernel(h->k_jvp_inst, 1, 1, 1, 64, 1, 1, 0,
                                      h->stream, nullptr, config));
        return 0;
    });
}

int opty_hip_jacprod_vjp_shard(opty_hip_jacprod *h, const double *free_,
                               const double *w, double *out,
                               int64_t out_stride, double *tail_part,
                               int64_t node_begin, int64_t node_end) {
    if (!h || !free_ || !w || !out) return fail("null argument");
    if (h->d.num_tail > 0 && !tail_part)
        return fail("null tail_part, but the problem has %d tail entries",
                    h->d.num_tail);
    if (int rc = check_window(h, node_begin, node_end)) return rc;
    // the time nodes the window owns: the last window also owns node N - 1
    const int64_t owned = node_end - node_begin +
        (node_end > node_begin && node_end == (int64_t)h->ncn() ? 1 : 0);
    if (out_stride < owned)
        return fail("out_stride %lld < the %lld time nodes the window owns",
                    (long long)out_stride, (long long)owned);
    if (node_begin == node_end) {
        // nothing to evaluate: the window's share of the tail sums is zero
        if (int rc = borrowed_begin(h, OPTY_HIP_DEVICE, true)) return rc;
        if (h->d.num_tail > 0) {
            h->zero_tail.assign((size_t)h->d.num_tail, 0.0);
            HIP_TRY(hipMemcpyAsync(tail_part, h->zero_tail.data(),
                                   (size_t)h->d.num_tail*sizeof(double),
                                   hipMemcpyHostToDevice, h->stream));
        }
        return 0;
    }
    return run_window(h, free_, w, out, out_stride, tail_part, node_begin,
                      node_end, [&](void **config) -> int {
        HIP_TRY(hipModuleLaunchKernel(
            h->k_vjp, (unsigned)h->vjp_blocks(node_begin, node_end),
            (unsigned)h->d.vjp_strips, 1, 64, 1, 1, 0, h->stream, nullptr,
            config));
        if (h->d.num_tail > 0 || h->d.nnz_inst > 0)
            HIP_TRY(hipModuleLaunchKernel(h->k_vjp_fin, 1, 1, 1, 64, 1, 1, 0,
                                          h->stream, nullptr, config));
        return 0;
    });
}

int opty_hip_jacprod_block_create(opty_hip_problem *p,
                                  const opty_hip_jacprod_block_desc *desc,
                                  const char *code_object_path,
                                  opty_hip_jacprod_block **out) {
    if (!p || !desc || !code_object_path || !out)
        return fail("null argument");
    if (desc->width != 2 && desc->width != 4)
        return fail("block width %d is neither 2 nor 4", desc->width);
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
    auto *h = new opty_hip_jacprod_block;
    h->d = *desc;
    if (int rc = borrowed_create(
            h, p, code_object_path,
            {{&h->k_jvp, "opty_jvp_block", true},
             {&h->k_jvp_inst, "opty_jvp_block_inst", true},
             {&h->k_vjp, "opty_vjp_block", true},
             {&h->k_vjp_fin, "opty_vjp_block_fin", true}},
            nullptr)) {
        delete h;
        return rc;
    }
    if (desc->num_tail > 0) {
        // one partial per block of opty_vjp_block, tail column and column
        hipError_t m = hipMalloc(
            (void **)&h->d_part,
            (size_t)desc->num_tail*(size_t)desc->width*
                (size_t)h->vjp_blocks()*sizeof(double));
        if (m != hipSuccess) {
            (void)hipGetLastError();
            (void)opty_hip_jacprod_block_destroy(h);
            return fail("hipMalloc of the partials failed: %s",
                        hipGetErrorString(m));
        }
    }
    *out = h;
    return 0;
}

int opty_hip_jacprod_block_destroy(opty_hip_jacprod_block *h) {
    if (!h) return 0;
    borrowed_destroy(h, {h->d_part, h->d_free, h->d_vec, h->d_out});
    delete h;
    return 0;
}

int32_t opty_hip_jacprod_block_width(const opty_hip_jacprod_block *h) {
    return h ? h->d.width : -1;
}

int opty_hip_jacprod_block_jvp(opty_hip_jacprod_block *h, const double *free_,
                               const double *V, int64_t ldv,
                               double *Y, int64_t ldy,
                               int32_t ncols, int32_t mem) {
    if (!h) return fail("null argument");
    opty_hip_problem *p = h->p;
    const long long nblk = (h->ncn() + 63)/64;
    return run_block(h, free_, V, "v", ldv, (size_t)p->num_free(), Y, "y",
                     ldy, (size_t)p->num_con(), ncols, mem,
                     [&](void **config) -> int {
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

int opty_hip_jacprod_block_vjp(opty_hip_jacprod_block *h, const double *free_,
                               const double *W, int64_t ldw,
                               double *G, int64_t ldg,
                               int32_t ncols, int32_t mem) {
    if (!h) return fail("null argument");
    opty_hip_problem *p = h->p;
    return run_block(h, free_, W, "w", ldw, (size_t)p->num_con(), G, "g",
                     ldg, (size_t)p->num_free(), ncols, mem,
                     [&](void **config) -> int {
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
