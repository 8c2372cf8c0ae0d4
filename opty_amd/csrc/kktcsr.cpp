// kktcsr.cpp -- the augmented-system handle of libopty_hip.so: the lower
// triangle of
//
//     K = [[ W + diag(sigma) + delta_w I ,  J^T        ],
//          [ J                           ,  -delta_c I ]]
//
// as ONE canonical CSR matrix over n + m rows (n = num_free, m =
// num_constraints), assembled on the device from the Hessian's triplets and
// the values of the CSR Jacobian (include/opty_hip.h, "Augmented system as
// CSR"; kkt_csr_structure / assemble_kkt_csr of codegen/program.py are the host
// statement).  Every diagonal is stored, last in its row, so that delta_w and
// delta_c can change between two factorisations without a new structure.
//
//   row r < n:  row r of the CSR Hessian WITH every diagonal pair
//       (opty_hip_hesscsr_create_with_diagonal).  These rows come first, so
//       the W part of K is data[0 .. nnzW) in exactly that handle's layout:
//       opty_hesscsr / opty_hesscsr_fin write it straight into data, no copy.
//   row n + j*(N-1) + i:  the L_j values of row (j, i) of the Jacobian
//       (jac[S_j*(N-1) + i*L_j + c]), then the diagonal: L_j + 1 values at
//       nnzW + (S_j + j)*(N-1) + i*(L_j + 1).
//   row n + M*(N-1) + k:  the entries of instance constraint k, then the
//       diagonal.
//
// Kernels.  opty_kkt_diag: lane = free row, data[at] = (data[at] + sigma[r]) +
// delta_w with `at` the row's last slot (one index read per row), behind the
// compression on the same stream.  opty_kkt_jrows: the source of equation j is
// one span of (N-1) L_j doubles, its destination one span of (N-1)(L_j + 1)
// doubles; the destination is swept flat in TILES of kTile doubles (a table
// of tiles built at create; one launch for all equations, a capped grid with
// a stride loop), consecutive lanes store consecutive 16-byte pairs counted
// from a 16-byte boundary -- an odd start or end of a span is one 8-byte
// store --; (row, c) of an element advance incrementally: one 32-bit division
// per lane and tile, none per element, no index is read from memory per
// element.  Element t = row*(L_j + 1) + c takes src[t - row] for c < L_j and
// 0.0 - delta_c for c == L_j.  opty_kkt_inst: lane = stored value of the
// instance rows, from a table built at create.
//
// Every element of data is stored exactly once (the W diagonals: once by the
// compression, then updated in place by opty_kkt_diag); no atomics; nothing
// outside data and the handle's staging buffers is written; nothing depends on
// anything but the inputs: the same bits in every call and for both memory
// kinds.
#include "opty_internal.h"

#include <cstdint>
#include <tuple>

using namespace opty;

namespace {

constexpr int kThreads = 256;
constexpr int kUnroll = 4;                      // pairs per lane and tile
constexpr int kTile = 2*kThreads*kUnroll;       // doubles of a tile
constexpr int kMaxBlocks = 2048;                // grid cap of the stride loops

// lane = free row
__global__ void __launch_bounds__(kThreads)
opty_kkt_diag(const long long *at, const double *sigma, double delta_w,
              double *data, long long n) {
    const long long stride = (long long)gridDim.x*kThreads;
    for (long long r = (long long)blockIdx.x*kThreads + threadIdx.x; r < n;
         r += stride) {
        const long long k = at[r];
        const double s = sigma ? sigma[r] : 0.0;
        data[k] = (data[k] + s) + delta_w;
    }
}

struct JrowsArgs {
    const double *jac;          // the Jacobian's values
    double *out;                // data + nnzW
    const int *teq;             // equation of tile w
    const long long *tu0;       // its first element of the equation's span,
    const long long *trow;      // ... a multiple of kTile, that element's row
    const int *tcol;            // ... and column
    const long long *edst;      // first destination element of equation j
    const long long *esrc;      // first source element: S_j*(N-1)
    const int *eL;              // L_j
    long long ncn, ntiles;
    double diag;                // 0.0 - delta_c
};

// Elements are counted from the 16-byte boundary at or before the span's
// start: u = t + ph, ph = 1 when the span starts 8 bytes off.  A lane owns
// the pairs u0 + 2*(lane + kThreads*k), k < kUnroll.
__global__ void __launch_bounds__(kThreads)
opty_kkt_jrows(JrowsArgs a) {
    typedef double d2 __attribute__((ext_vector_type(2)));
    for (long long w = blockIdx.x; w < a.ntiles; w += gridDim.x) {
        const int j = a.teq[w];
        const int L = a.eL[j], L1 = L + 1;
        const long long span = a.ncn*L1;
        double *dst = a.out + a.edst[j];
        const double *src = a.jac + a.esrc[j];
        const int ph =
            (int)((reinterpret_cast<unsigned long long>(dst) >> 3) & 1);
        const int e = 2*(int)threadIdx.x;
        const int q = e/L1;
        int c = a.tcol[w] + (e - q*L1);
        long long row = a.trow[w] + q;
        if (c >= L1) {
            c -= L1;
            ++row;
        }
        if (ph && --c < 0) {
            c = L;
            --row;
        }
        long long t = a.tu0[w] + e - ph;
        constexpr int step = 2*kThreads;
        const int dq = step/L1, dr = step - dq*L1;
        double v0[kUnroll], v1[kUnroll];
#pragma unroll
        for (int k = 0; k < kUnroll; ++k) {
            int c1 = c + 1;
            long long row1 = row;
            if (c1 > L) {
                c1 = 0;
                ++row1;
            }
            const bool ok0 = t >= 0 && t < span, ok1 = t + 1 < span;
            v0[k] = ok0 && c < L ? src[t - row] : a.diag;
            v1[k] = ok1 && c1 < L ? src[t + 1 - row1] : a.diag;
            t += step;
            row += dq;
            c += dr;
            if (c >= L1) {
                c -= L1;
                ++row;
            }
        }
        t -= (long long)kUnroll*step;
#pragma unroll
        for (int k = 0; k < kUnroll; ++k) {
            const bool ok0 = t >= 0 && t < span, ok1 = t + 1 < span;
            if (ok0 && ok1) {
                d2 v;
                v.x = v0[k];
                v.y = v1[k];
                *reinterpret_cast<d2 *>(dst + t) = v;
            } else if (ok0) {
                dst[t] = v0[k];
            } else if (ok1) {
                dst[t + 1] = v1[k];
            }
            t += step;
        }
    }
}

// lane = stored value of the instance rows: entry src[m] of the Jacobian's
// instance tail, or (src[m] < 0) the diagonal
__global__ void __launch_bounds__(64)
opty_kkt_inst(const int *src, const double *tail, double diag, double *out,
              int count) {
    const int m = blockIdx.x*64 + threadIdx.x;
    if (m >= count) return;
    const int s = src[m];
    out[m] = s >= 0 ? tail[s] : diag;
}

// where wrt column k of the block lives in `free` (column_side of
// codegen/program.py): (row, off) -- free index row*N + i + off -- or
// (-1, j) -- the tail entry (n + q)*N + j
std::pair<int, int> column_side(const opty_hip_desc &d, int k) {
    const bool be = d.method == OPTY_HIP_BACKWARD_EULER;
    const int n = d.n, q = d.q, cur = be ? 1 : 0, adj = be ? 0 : 1;
    if (k < n) return {k, cur};
    if (k < 2*n) return {k - n, adj};
    const int j = k - 2*n;
    if (j < q) return {n + j, cur};
    if (!be && j < 2*q) return {n + j - q, adj};
    return {-1, j - (be ? q : 2*q)};
}

bool overlaps(const void *a, size_t na, const void *b, size_t nb) {
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a0 < b0 + nb*sizeof(double) && b0 < a0 + na*sizeof(double);
}

}  // namespace

struct opty_hip_kktcsr : Borrowed {
    opty_hip_hesscsr *hess = nullptr;   // W with every diagonal (owned)
    int64_t nnz_w = 0, nnz_k = 0, nnz_jac = 0, nnz_triplets = 0;
    long long ntiles = 0;
    int ninst_out = 0;
    // what opty_hip_kktcsr_structure walks
    std::vector<int> eS, eL;                        // per equation
    std::vector<std::pair<int, int>> side;          // per block entry
    std::vector<int64_t> inst_row, inst_col;        // local row, free column
    int *d_teq = nullptr, *d_tcol = nullptr, *d_eL = nullptr,
        *d_isrc = nullptr;
    long long *d_tu0 = nullptr, *d_trow = nullptr, *d_edst = nullptr,
              *d_esrc = nullptr, *d_diagat = nullptr;
    // staging for host callers
    double *d_hval = nullptr, *d_jval = nullptr, *d_sigma = nullptr,
           *d_data = nullptr;
    long long ncn() const { return p->d.N - 1; }
};

extern "C" {

int opty_hip_kktcsr_create(opty_hip_problem *p,
                           const opty_hip_hessmv_desc *desc,
                           opty_hip_kktcsr **out) {
    if (!p || !desc || !out) return fail("null argument");
    if (p->d.layout != OPTY_HIP_LAYOUT_CSR)
        return fail("the augmented system as CSR needs the Jacobian in "
                    "OPTY_HIP_LAYOUT_CSR (jacobian_layout='csr'); the "
                    "problem handle has layout %d", p->d.layout);
    if (int rc = check_hessmv_desc(p, desc)) return rc;
    const int M = p->d.M, P = p->d.P, num_inst = p->d.num_inst,
              nnz_inst = p->d.nnz_inst;
    if (p->block_jk.size() != 2*(size_t)P)
        return fail("the CSR block pattern was never set "
                    "(opty_hip_set_block_pattern)");
    if (num_inst > 0 && !p->have_inst)
        return fail("instance indices were never set");
    const long long N = p->d.N, ncn = N - 1;
    const int64_t nfree = p->num_free();

    auto *h = new opty_hip_kktcsr;
    h->p = p;
    h->device = p->d.device;
    auto refuse = [&](int rc) {
        (void)opty_hip_kktcsr_destroy(h);
        return rc;
    };
    // rows of the block: grouped by equation, ascending (checked by
    // opty_hip_set_block_pattern); the columns of a row ascend at every node
    // when their sides do (trajectory rows by row then slot, the tail last)
    h->eS.assign(M, 0);
    h->eL.assign(M, 0);
    for (int e = 0; e < P; ++e) {
        const int j = p->block_jk[2*e];
        if (h->eL[j]++ == 0) h->eS[j] = e;
        h->side.push_back(column_side(p->d, p->block_jk[2*e + 1]));
        if (e > 0 && p->block_jk[2*(e - 1)] == j) {
            auto key = [](std::pair<int, int> s) {
                return s.first < 0 ? std::make_tuple(1, s.second, 0)
                                   : std::make_tuple(0, s.first, s.second);
            };
            if (!(key(h->side[e - 1]) < key(h->side[e])))
                return refuse(fail("block pattern entry %d: the columns of "
                                   "equation %d do not ascend", e, j));
        }
    }
    {
        int S = 0;
        for (int j = 0; j < M; ++j) {
            if (h->eL[j] == 0) h->eS[j] = S;
            S = h->eS[j] + h->eL[j];
        }
    }
    // the instance tail: sorted by row, then column
    std::vector<int> icount(num_inst, 0);
    for (int k = 0; k < nnz_inst; ++k) {
        const int64_t r = p->inst_rows_host[k] - (int64_t)M*ncn,
                      c = p->inst_cols_host[k];
        if (r < 0 || r >= num_inst || c < 0 || c >= nfree)
            return refuse(fail("instance entry %d: (%lld, %lld) outside the "
                               "problem", k, (long long)p->inst_rows_host[k],
                               (long long)c));
        if (k > 0 && (r < h->inst_row[k - 1] ||
                      (r == h->inst_row[k - 1] && c <= h->inst_col[k - 1])))
            return refuse(fail("instance entry %d: the instance entries are "
                               "not sorted by row, then column", k));
        h->inst_row.push_back(r);
        h->inst_col.push_back(c);
        ++icount[(size_t)r];
    }

    if (int rc = opty_hip_hesscsr_create_with_diagonal(p, desc, &h->hess))
        return refuse(rc);
    h->nnz_triplets = opty_hip_hesscsr_nnz(h->hess);
    h->nnz_w = opty_hip_hesscsr_nnz_unique(h->hess);
    h->nnz_jac = p->nnz();
    const long long jrows = (long long)(P + M)*ncn;     // values of J's rows
    h->ninst_out = nnz_inst + num_inst;
    h->nnz_k = h->nnz_w + jrows + h->ninst_out;

    // last slot of every free row
    std::vector<long long> diagat((size_t)nfree);
    {
        std::vector<int64_t> ptr((size_t)nfree + 1),
                             idx((size_t)h->nnz_w);
        if (int rc = opty_hip_hesscsr_structure(h->hess, ptr.data(),
                                                idx.data(), OPTY_HIP_HOST))
            return refuse(rc);
        for (size_t r = 0; r < (size_t)nfree; ++r) {
            diagat[r] = ptr[r + 1] - 1;
            if (ptr[r + 1] <= ptr[r] || idx[(size_t)diagat[r]] != (int64_t)r)
                return refuse(fail("row %zu of the Hessian does not end with "
                                   "its diagonal", r));
        }
    }
    // tiles of the equations' destination spans: one element more than the
    // span, for a span that starts 8 bytes off a 16-byte boundary
    std::vector<int> teq, tcol;
    std::vector<long long> tu0, trow, edst(M), esrc(M);
    for (int j = 0; j < M; ++j) {
        const long long L1 = h->eL[j] + 1, span = ncn*L1;
        edst[j] = ((long long)h->eS[j] + j)*ncn;
        esrc[j] = (long long)h->eS[j]*ncn;
        // (every span stays inside data and inside the Jacobian's values)
        if (edst[j] < 0 || edst[j] + span > jrows ||
            esrc[j] + ncn*h->eL[j] > (long long)P*ncn)
            return refuse(fail("equation %d leaves the %lld values of the "
                               "Jacobian rows", j, jrows));
        for (long long u0 = 0; u0 < span + 1; u0 += kTile) {
            teq.push_back(j);
            tu0.push_back(u0);
            trow.push_back(u0/L1);
            tcol.push_back((int)(u0 % L1));
        }
    }
    h->ntiles = (long long)teq.size();
    // the stored values of the instance rows
    std::vector<int> isrc;
    for (int k = 0, s = 0; k < num_inst; ++k) {
        for (int t = 0; t < icount[k]; ++t) isrc.push_back(s++);
        isrc.push_back(-1);
    }
    if ((int)isrc.size() != h->ninst_out)
        return refuse(fail("the instance rows hold %zu values, not %d",
                           isrc.size(), h->ninst_out));
    for (long long at : diagat)
        if (at < 0 || at >= h->nnz_w)
            return refuse(fail("a diagonal at %lld leaves the %lld values of "
                               "the Hessian block", at, (long long)h->nnz_w));

    auto device_side = [&]() -> int {
        if (int rc = use_device(p)) return rc;
        if (int rc = upload(&h->d_teq, teq.data(), teq.size())) return rc;
        if (int rc = upload(&h->d_tu0, tu0.data(), tu0.size())) return rc;
        if (int rc = upload(&h->d_trow, trow.data(), trow.size())) return rc;
        if (int rc = upload(&h->d_tcol, tcol.data(), tcol.size())) return rc;
        if (int rc = upload(&h->d_edst, edst.data(), edst.size())) return rc;
        if (int rc = upload(&h->d_esrc, esrc.data(), esrc.size())) return rc;
        if (int rc = upload(&h->d_eL, h->eL.data(), h->eL.size())) return rc;
        if (int rc = upload(&h->d_isrc, isrc.data(), isrc.size())) return rc;
        return upload(&h->d_diagat, diagat.data(), diagat.size());
    };
    if (int rc = device_side()) return refuse(rc);
    *out = h;
    return 0;
}

int opty_hip_kktcsr_destroy(opty_hip_kktcsr *h) {
    if (!h) return 0;
    borrowed_destroy(h, {h->d_teq, h->d_tu0, h->d_trow, h->d_tcol, h->d_edst,
                         h->d_esrc, h->d_eL, h->d_isrc, h->d_diagat,
                         h->d_hval, h->d_jval, h->d_sigma, h->d_data});
    (void)opty_hip_hesscsr_destroy(h->hess);
    delete h;
    return 0;
}

int64_t opty_hip_kktcsr_nnz(const opty_hip_kktcsr *h) {
    return h ? h->nnz_k : -1;
}

int64_t opty_hip_kktcsr_nnz_hessian(const opty_hip_kktcsr *h) {
    return h ? h->nnz_w : -1;
}

int64_t opty_hip_kktcsr_nnz_triplets(const opty_hip_kktcsr *h) {
    return h ? h->nnz_triplets : -1;
}

int opty_hip_kktcsr_structure(opty_hip_kktcsr *h, int64_t *indptr,
                              int64_t *indices, int32_t mem) {
    if (!h || !indptr || !indices) return fail("null argument");
    if (int rc = borrowed_begin(h, mem, false)) return rc;
    const opty_hip_problem *p = h->p;
    const long long N = p->d.N, ncn = N - 1;
    const int M = p->d.M;
    const size_t n = (size_t)p->num_free(), m = (size_t)p->num_con();
    const int64_t tail = (int64_t)(p->d.n + p->d.q)*N;
    std::vector<int64_t> ptr(n + m + 1), idx((size_t)h->nnz_k);
    if (int rc = opty_hip_hesscsr_structure(h->hess, ptr.data(), idx.data(),
                                            OPTY_HIP_HOST))
        return rc;
    size_t at = (size_t)h->nnz_w, row = n;
    for (int j = 0; j < M; ++j)
        for (long long i = 0; i < ncn; ++i) {
            ptr[row] = (int64_t)at;
            for (int e = h->eS[j]; e < h->eS[j] + h->eL[j]; ++e)
                idx[at++] = h->side[e].first >= 0
                    ? (int64_t)h->side[e].first*N + i + h->side[e].second
                    : tail + h->side[e].second;
            idx[at++] = (int64_t)row++;
        }
    for (size_t k = 0, s = 0; k < (size_t)p->d.num_inst; ++k) {
        ptr[row] = (int64_t)at;
        for (; s < h->inst_row.size() && h->inst_row[s] == (int64_t)k; ++s)
            idx[at++] = h->inst_col[s];
        idx[at++] = (int64_t)row++;
    }
    ptr[n + m] = (int64_t)at;
    if (at != (size_t)h->nnz_k || row != n + m)
        return fail("the CSR structure has %zu columns in %zu rows, the "
                    "handle counted %lld in %zu", at, row,
                    (long long)h->nnz_k, n + m);
    if (mem == OPTY_HIP_HOST) {
        std::memcpy(indptr, ptr.data(), ptr.size()*sizeof(int64_t));
        std::memcpy(indices, idx.data(), idx.size()*sizeof(int64_t));
        return 0;
    }
    // (the vectors end with this call: the copies are waited for)
    HIP_TRY(hipMemcpyAsync(indptr, ptr.data(), ptr.size()*sizeof(int64_t),
                           hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(indices, idx.data(), idx.size()*sizeof(int64_t),
                           hipMemcpyHostToDevice, h->stream));
    return host_done(h);
}

}  // extern "C"

// Both assemble entry points.  ev: null, or five events that are recorded
// before the compression and after each of the four stages.
static int assemble_impl(opty_hip_kktcsr *h, const double *hess_values,
                         const double *jac_values, const double *sigma,
                         double delta_w, double delta_c, double *data,
                         int32_t mem, hipEvent_t *ev) {
    if (!h || !hess_values || !jac_values || !data)
        return fail("null argument");
    const size_t nh = (size_t)h->nnz_triplets, nj = (size_t)h->nnz_jac,
                 nk = (size_t)h->nnz_k, n = (size_t)h->p->num_free();
    if (overlaps(data, nk, hess_values, nh))
        return fail("data (%zu values) overlaps the %zu values of the "
                    "Hessian", nk, nh);
    if (overlaps(data, nk, jac_values, nj))
        return fail("data (%zu values) overlaps the %zu values of the "
                    "Jacobian", nk, nj);
    if (sigma && overlaps(data, nk, sigma, n))
        return fail("data (%zu values) overlaps the %zu values of sigma",
                    nk, n);
    if (int rc = borrowed_begin(h, mem, false)) return rc;
    double *out = data;
    if (mem == OPTY_HIP_HOST) {
        if (int rc = stage_in(h, &hess_values, &h->d_hval, nh,
                              std::max<size_t>(1, nh)))
            return rc;
        if (int rc = stage_in(h, &jac_values, &h->d_jval, nj,
                              std::max<size_t>(1, nj)))
            return rc;
        if (sigma)
            if (int rc = stage_in(h, &sigma, &h->d_sigma, n,
                                  std::max<size_t>(1, n)))
                return rc;
        if (int rc = ensure(&h->d_data, nk)) return rc;
        out = h->d_data;
    }
    // the W part, straight into data[0 .. nnzW)
    if (ev) HIP_TRY(hipEventRecord(ev[0], h->stream));
    if (int rc = opty_hip_hesscsr_compress(h->hess, hess_values, out,
                                           OPTY_HIP_DEVICE))
        return rc;
    if (ev) HIP_TRY(hipEventRecord(ev[1], h->stream));
    const double diag = 0.0 - delta_c;
    if (n > 0) {
        const unsigned grid = (unsigned)std::min<size_t>(
            kMaxBlocks, (n + kThreads - 1)/kThreads);
        hipLaunchKernelGGL(opty_kkt_diag, dim3(grid), dim3(kThreads), 0,
                           h->stream, h->d_diagat, sigma, delta_w, out,
                           (long long)n);
        HIP_TRY(hipGetLastError());
    }
    if (ev) HIP_TRY(hipEventRecord(ev[2], h->stream));
    if (h->ntiles > 0) {
        JrowsArgs a{};
        a.jac = jac_values;
        a.out = out + h->nnz_w;
        a.teq = h->d_teq;
        a.tu0 = h->d_tu0;
        a.trow = h->d_trow;
        a.tcol = h->d_tcol;
        a.edst = h->d_edst;
        a.esrc = h->d_esrc;
        a.eL = h->d_eL;
        a.ncn = h->ncn();
        a.ntiles = h->ntiles;
        a.diag = diag;
        const unsigned grid = (unsigned)std::min<long long>(kMaxBlocks,
                                                            h->ntiles);
        hipLaunchKernelGGL(opty_kkt_jrows, dim3(grid), dim3(kThreads), 0,
                           h->stream, a);
        HIP_TRY(hipGetLastError());
    }
    if (ev) HIP_TRY(hipEventRecord(ev[3], h->stream));
    if (h->ninst_out > 0) {
        hipLaunchKernelGGL(opty_kkt_inst,
                           dim3((unsigned)((h->ninst_out + 63)/64)), dim3(64),
                           0, h->stream, h->d_isrc,
                           jac_values + (size_t)h->p->P()*h->ncn(), diag,
                           out + (nk - (size_t)h->ninst_out), h->ninst_out);
        HIP_TRY(hipGetLastError());
    }
    if (ev) HIP_TRY(hipEventRecord(ev[4], h->stream));
    if (mem == OPTY_HIP_HOST) {
        if (int rc = stage_out(h, data, h->d_data, nk*sizeof(double)))
            return rc;
        return host_done(h);
    }
    return 0;
}

extern "C" {

int opty_hip_kktcsr_assemble(opty_hip_kktcsr *h, const double *hess_values,
                             const double *jac_values, const double *sigma,
                             double delta_w, double delta_c, double *data,
                             int32_t mem) {
    return assemble_impl(h, hess_values, jac_values, sigma, delta_w, delta_c,
                         data, mem, nullptr);
}

int opty_hip_kktcsr_assemble_timed(opty_hip_kktcsr *h,
                                   const double *hess_values,
                                   const double *jac_values,
                                   const double *sigma, double delta_w,
                                   double delta_c, double *data,
                                   float *stage_ms) {
    if (!stage_ms) return fail("null argument");
    if (!h) return fail("null argument");
    if (int rc = use_device(h->p)) return rc;
    hipEvent_t ev[5] = {};
    int rc = 0;
    for (hipEvent_t &e : ev)
        if (!rc && hipEventCreate(&e) != hipSuccess) {
            (void)hipGetLastError();
            rc = fail("hipEventCreate failed");
        }
    if (!rc)
        rc = assemble_impl(h, hess_values, jac_values, sigma, delta_w,
                           delta_c, data, OPTY_HIP_DEVICE, ev);
    if (!rc && hipStreamSynchronize(sync_target(h->stream)) != hipSuccess) {
        (void)hipGetLastError();
        rc = fail("hipStreamSynchronize failed");
    }
    for (int k = 0; k < 4 && !rc; ++k)
        if (hipEventElapsedTime(stage_ms + k, ev[k], ev[k + 1]) !=
            hipSuccess) {
            (void)hipGetLastError();
            rc = fail("hipEventElapsedTime failed");
        }
    for (hipEvent_t e : ev)
        if (e) (void)hipEventDestroy(e);
    return rc;
}

}  // extern "C"
