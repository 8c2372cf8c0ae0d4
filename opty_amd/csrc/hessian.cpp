// hessian.cpp -- the Hessian handle of libopty_hip.so: the exact Hessian of
// the constraint Lagrangian, sum_k lagrange_k d2 con_k / d free^2, lower
// triangle, as triplets (include/opty_hip.h, "exact Hessian").
//
// The handle borrows its problem handle (device, stream, known parameters,
// known trajectories, h, instance atom indices): one copy of the known data,
// and what opty_hip_set_known_* installs is what the next call reads.  The
// generated code object exports `opty_hess` (lane = constraint node, grid.y =
// strips of the per-node entries) and `opty_hess_inst` (one lane, the
// instance constraints' entries after the node blocks).  Both take a window
// [wa, wb) of the constraint nodes: the whole problem is [0, N-1), a rank of a
// node-sharded problem launches its own (opty_hip_eval_hess_shard).
#include "opty_internal.h"

#include <cstdint>

using namespace opty;

namespace {

// The packed kernarg buffer of opty_hess / opty_hess_inst; must match
// HESS_PARAMS in opty_amd/codegen/emit_hessian.py.
struct HessArgs {
    const double *free_;
    const double *known_traj;
    const double *params;
    const double *lam;
    const long long *inst_idx;
    double *hess;
    double h;
    long long N;
    long long wa, wb;   // the window of constraint nodes; hess: its first node
    double *tail;       // opty_hess_inst: the nnz_inst instance entries
};
static_assert(sizeof(HessArgs) == 88, "HessArgs must match HESS_PARAMS");

// Closed-form indices: entry e of constraint node i has the global indices
// side(pattern[4e], pattern[4e+1]) and side(pattern[4e+2], pattern[4e+3]),
// side(row, off) = row*N + i + off, or tail + off for row == -1.  The
// instance entries follow the node blocks (a table; the last block).  One
// block per node row: consecutive lanes write consecutive int64s.
__global__ void __launch_bounds__(256)
opty_hess_indices_kernel(const int *pattern, int PH, long long N,
                         long long ncn, long long tail, const long long *irows,
                         const long long *icols, int nnz_inst,
                         long long *rows, long long *cols, long long wa,
                         long long wb) {
    // [wa, wb): the window of nodes; rows / cols start at its first node.
    // The instance block exists in the whole-problem launch only (wb == ncn,
    // wa == 0), one block past the nodes.
    const long long i = wa + blockIdx.x;
    if (i < wb) {
        const long long at = (i - wa)*PH;
        for (int e = threadIdx.x; e < PH; e += blockDim.x) {
            const int ra = pattern[4*e], oa = pattern[4*e + 1];
            const int rb = pattern[4*e + 2], ob = pattern[4*e + 3];
            rows[at + e] = ra >= 0 ? (long long)ra*N + i + oa : tail + oa;
            cols[at + e] = rb >= 0 ? (long long)rb*N + i + ob : tail + ob;
        }
    } else {
        for (int t = threadIdx.x; t < nnz_inst; t += blockDim.x) {
            rows[ncn*PH + t] = irows[t];
            cols[ncn*PH + t] = icols[t];
        }
    }
}

}  // namespace

struct opty_hip_hessian : Borrowed {
    opty_hip_hessian_desc d{};
    hipFunction_t k_hess = nullptr, k_inst = nullptr;
    int *d_pattern = nullptr;
    long long *d_irows = nullptr, *d_icols = nullptr;
    // staging for host callers
    double *d_free = nullptr, *d_lam = nullptr, *d_hess = nullptr;
    long long *d_rows = nullptr, *d_cols = nullptr;
    int64_t ncn() const { return p->d.N - 1; }
    int64_t nnz() const { return (int64_t)d.PH*ncn() + d.nnz_inst; }
};

namespace {

// Enqueues opty_hess over the window [wa, wb) -- `hess`: the entries of node
// wa -- and / or opty_hess_inst into `tail` (null: not launched).
int launch_hess(opty_hip_hessian *h, const double *free_, const double *lam,
                double *hess, long long wa, long long wb, double *tail) {
    HessArgs a{};
    borrowed_args(&a, h->p, free_);
    a.lam = lam;
    a.hess = hess;
    a.wa = wa;
    a.wb = wb;
    a.tail = tail;
    size_t size = sizeof a;
    void *config[] = {HIP_LAUNCH_PARAM_BUFFER_POINTER, &a,
                      HIP_LAUNCH_PARAM_BUFFER_SIZE, &size,
                      HIP_LAUNCH_PARAM_END};
    const long long nblk = (wb - wa + 63)/64;
    if (h->d.PH > 0 && nblk > 0)
        HIP_TRY(hipModuleLaunchKernel(h->k_hess, (unsigned)nblk,
                                      (unsigned)h->d.strips, 1, 64, 1, 1, 0,
                                      h->stream, nullptr, config));
    if (h->d.nnz_inst > 0 && tail)
        HIP_TRY(hipModuleLaunchKernel(h->k_inst, 1, 1, 1, 64, 1, 1, 0,
                                      h->stream, nullptr, config));
    return 0;
}

// The window check of the windowed entry points: the offending number is in
// the message.
int check_hess_window(const opty_hip_hessian *h, int64_t a, int64_t b) {
    if (a < 0) return fail("node_begin %lld < 0", (long long)a);
    if (b > h->ncn())
        return fail("node_end %lld > the %lld constraint nodes",
                    (long long)b, (long long)h->ncn());
    if (a > b)
        return fail("node_begin %lld > node_end %lld", (long long)a,
                    (long long)b);
    return 0;
}

}  // namespace

extern "C" {

int opty_hip_hessian_create(opty_hip_problem *p,
                            const opty_hip_hessian_desc *desc,
                            const char *code_object_path,
                            opty_hip_hessian **out) {
    if (!p || !desc || !code_object_path || !out)
        return fail("null argument");
    if (desc->PH < 0 || desc->nnz_inst < 0 || desc->strips < 1)
        return fail("bad Hessian descriptor (PH %d, nnz_inst %d, strips %d)",
                    desc->PH, desc->nnz_inst, desc->strips);
    if (desc->PH > 0 && !desc->pattern) return fail("null index pattern");
    if (desc->nnz_inst > 0 && (!desc->inst_rows || !desc->inst_cols))
        return fail("null instance indices");
    if (desc->nnz_inst > 0 && p->d.num_inst == 0)
        return fail("instance entries but the problem has no instance "
                    "constraints");
    if (int rc = use_device(p)) return rc;
    auto *h = new opty_hip_hessian;
    h->d = *desc;
    h->d.pattern = nullptr;
    h->d.inst_rows = h->d.inst_cols = nullptr;
    if (int rc = borrowed_create(
            h, p, code_object_path,
            {{&h->k_hess, "opty_hess", desc->PH > 0},
             {&h->k_inst, "opty_hess_inst", desc->nnz_inst > 0}},
            "opty_hess/opty_hess_inst")) {
        delete h;
        return rc;
    }
    auto upload = [&]() -> int {
        if (desc->PH > 0) {
            HIP_TRY(hipMalloc((void **)&h->d_pattern,
                              (size_t)4*desc->PH*sizeof(int)));
            HIP_TRY(hipMemcpy(h->d_pattern, desc->pattern,
                              (size_t)4*desc->PH*sizeof(int),
                              hipMemcpyHostToDevice));
        }
        if (desc->nnz_inst > 0) {
            const size_t b = (size_t)desc->nnz_inst*sizeof(long long);
            HIP_TRY(hipMalloc((void **)&h->d_irows, b));
            HIP_TRY(hipMalloc((void **)&h->d_icols, b));
            HIP_TRY(hipMemcpy(h->d_irows, desc->inst_rows, b,
                              hipMemcpyHostToDevice));
            HIP_TRY(hipMemcpy(h->d_icols, desc->inst_cols, b,
                              hipMemcpyHostToDevice));
        }
        return 0;
    };
    if (int rc = upload()) {
        (void)opty_hip_hessian_destroy(h);
        return rc;
    }
    *out = h;
    return 0;
}

int opty_hip_hessian_destroy(opty_hip_hessian *h) {
    if (!h) return 0;
    borrowed_destroy(h, {h->d_pattern, h->d_irows, h->d_icols, h->d_free,
                         h->d_lam, h->d_hess, h->d_rows, h->d_cols});
    delete h;
    return 0;
}

int64_t opty_hip_hessian_nnz(const opty_hip_hessian *h) {
    return h ? h->nnz() : -1;
}

int opty_hip_eval_hess(opty_hip_hessian *h, const double *free_,
                       const double *lagrange, double *hess, int32_t mem) {
    if (!h || !free_ || !lagrange || !hess) return fail("null argument");
    // an even PH is flushed with 16-byte stores at hess + (even offset)
    // (opty_flush16): the caller's device pointer has to allow them
    if (mem == OPTY_HIP_DEVICE && h->d.PH > 0 && h->d.PH % 2 == 0 &&
        (reinterpret_cast<uintptr_t>(hess) & 15) != 0)
        return fail("hess (%p) must be 16-byte aligned in device memory when "
                    "PH (%d) is even", (void *)hess, h->d.PH);
    if (int rc = borrowed_begin(h, mem, true)) return rc;
    opty_hip_problem *p = h->p;
    const long long ncn = h->ncn();
    const size_t nfree = (size_t)p->num_free(), ncon = (size_t)p->num_con(),
                 nnz = (size_t)h->nnz();
    const double *lam = lagrange;
    double *dhess = hess;
    if (mem == OPTY_HIP_HOST) {
        if (int rc = stage_in(h, &free_, &h->d_free, nfree, nfree)) return rc;
        if (int rc = stage_in(h, &lam, &h->d_lam, ncon,
                              std::max<size_t>(1, ncon)))
            return rc;
        if (int rc = ensure(&h->d_hess, std::max<size_t>(1, nnz))) return rc;
        dhess = h->d_hess;
    }
    // the whole problem: every constraint node, the instance entries behind
    // the node blocks
    if (int rc = launch_hess(h, free_, lam, dhess, 0, ncn,
                             dhess + (size_t)ncn*(size_t)h->d.PH))
        return rc;
    if (mem == OPTY_HIP_HOST) {
        if (int rc = stage_out(h, hess, h->d_hess, nnz*sizeof(double)))
            return rc;
        return host_done(h);
    }
    return 0;
}

int opty_hip_hessian_indices(opty_hip_hessian *h, int64_t *rows,
                             int64_t *cols, int32_t mem) {
    if (!h || !rows || !cols) return fail("null argument");
    if (int rc = borrowed_begin(h, mem, false)) return rc;
    opty_hip_problem *p = h->p;
    const long long ncn = h->ncn();
    const size_t nnz = (size_t)h->nnz();
    long long *dr = (long long *)rows, *dc = (long long *)cols;
    if (mem == OPTY_HIP_HOST) {
        if (int rc = ensure(&h->d_rows, std::max<size_t>(1, nnz))) return rc;
        if (int rc = ensure(&h->d_cols, std::max<size_t>(1, nnz))) return rc;
        dr = h->d_rows;
        dc = h->d_cols;
    }
    const long long tail = (long long)(p->d.n + p->d.q)*p->d.N;
    const long long blocks = ncn + (h->d.nnz_inst > 0 ? 1 : 0);
    if (blocks > 0 && nnz > 0) {
        hipLaunchKernelGGL(opty_hess_indices_kernel, dim3((unsigned)blocks),
                           dim3(256), 0, h->stream, h->d_pattern, h->d.PH,
                           (long long)p->d.N, ncn, tail, h->d_irows,
                           h->d_icols, h->d.nnz_inst, dr, dc, 0LL, ncn);
        HIP_TRY(hipGetLastError());
    }
    if (mem == OPTY_HIP_HOST) {
        if (int rc = stage_out(h, rows, h->d_rows, nnz*sizeof(long long)))
            return rc;
        if (int rc = stage_out(h, cols, h->d_cols, nnz*sizeof(long long)))
            return rc;
        return host_done(h);
    }
    return 0;
}

int opty_hip_eval_hess_shard(opty_hip_hessian *h, const double *free_,
                             const double *lagrange, double *hess_shard,
                             int64_t node_begin, int64_t node_end) {
    if (!h || !free_ || !lagrange || !hess_shard)
        return fail("null argument");
    if (int rc = check_hess_window(h, node_begin, node_end)) return rc;
    // an even PH: 16-byte stores at hess_shard + (even offset); every in-place
    // window base global + node_begin*PH is aligned when the global base is
    if (h->d.PH > 0 && h->d.PH % 2 == 0 &&
        (reinterpret_cast<uintptr_t>(hess_shard) & 15) != 0)
        return fail("hess_shard (%p) must be 16-byte aligned in device memory "
                    "when PH (%d) is even", (void *)hess_shard, h->d.PH);
    if (int rc = borrowed_begin(h, OPTY_HIP_DEVICE, true)) return rc;
    if (node_begin == node_end) return 0;
    return launch_hess(h, free_, lagrange, hess_shard, node_begin, node_end,
                       nullptr);
}

int opty_hip_eval_hess_instance(opty_hip_hessian *h, const double *free_,
                                const double *lagrange, double *inst_out) {
    if (!h || !free_ || !lagrange) return fail("null argument");
    if (h->d.nnz_inst == 0) return 0;
    if (!inst_out) return fail("null argument");
    if (int rc = borrowed_begin(h, OPTY_HIP_DEVICE, true)) return rc;
    return launch_hess(h, free_, lagrange, nullptr, 0, 0, inst_out);
}

int opty_hip_hessian_indices_range(opty_hip_hessian *h, int64_t node_begin,
                                   int64_t node_end, int64_t *rows,
                                   int64_t *cols, int32_t mem) {
    if (!h || !rows || !cols) return fail("null argument");
    if (int rc = check_hess_window(h, node_begin, node_end)) return rc;
    if (int rc = borrowed_begin(h, mem, false)) return rc;
    opty_hip_problem *p = h->p;
    const long long count = node_end - node_begin;
    const size_t nnz = (size_t)count*(size_t)h->d.PH;
    if (nnz == 0) return 0;
    long long *dr = (long long *)rows, *dc = (long long *)cols;
    if (mem == OPTY_HIP_HOST) {
        // (the staging vectors of opty_hip_hessian_indices: the whole
        // problem's size, which no window exceeds)
        const size_t all = std::max<size_t>(1, (size_t)h->nnz());
        if (int rc = ensure(&h->d_rows, all)) return rc;
        if (int rc = ensure(&h->d_cols, all)) return rc;
        dr = h->d_rows;
        dc = h->d_cols;
    }
    const long long tail = (long long)(p->d.n + p->d.q)*p->d.N;
    hipLaunchKernelGGL(opty_hess_indices_kernel, dim3((unsigned)count),
                       dim3(256), 0, h->stream, h->d_pattern, h->d.PH,
                       (long long)p->d.N, (long long)h->ncn(), tail,
                       h->d_irows, h->d_icols, 0, dr, dc,
                       (long long)node_begin, (long long)node_end);
    HIP_TRY(hipGetLastError());
    if (mem == OPTY_HIP_HOST) {
        if (int rc = stage_out(h, rows, h->d_rows, nnz*sizeof(long long)))
            return rc;
        if (int rc = stage_out(h, cols, h->d_cols, nnz*sizeof(long long)))
            return rc;
        return host_done(h);
    }
    return 0;
}

}  // extern "C"
