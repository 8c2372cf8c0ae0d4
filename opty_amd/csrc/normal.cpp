// normal.cpp -- the normal-matrix handle of libopty_hip.so: a direct solve
// with
//
//     S = Jc[:, :T] diag(1/d[:T]) Jc[:, :T]^T + delta_c I
//
// (Jc: the M(N-1) collocation rows of the constraint Jacobian, T = (n+q)N the
// trajectory part of `free`).  Constraint node i touches only the time nodes
// i and i + 1, so, ordered by node, S is symmetric block TRIDIAGONAL with
// N - 1 diagonal blocks A_i of M x M and N - 2 couplings B_i = S[i+1, i]
// (include/opty_hip.h, "Normal matrix"; normal_blocks / normal_factor /
// normal_solve of codegen/program.py are the host statement).
//
// Factorisation: block cyclic reduction with Cholesky factors of the
// eliminated diagonal blocks -- a sparse Cholesky of S under an odd-even
// ordering, no pivoting.  Level l has n_l rows, n_0 = N - 1, n_{l+1} =
// ceil(n_l/2); rows 1, 3, 5, ... are eliminated, rows 0, 2, 4, ... survive as
// e = k/2; a level with one row is a plain Cholesky.  Eliminated row k:
//
//     L_k = chol(A_k),  U_k = L_k^-1 S[k, k-1],  V_k = L_k^-1 S[k, k+1]
//
// stored IN PLACE (L_k over A_k, U_k over B_{k-1}, V_k over B_k); survivors:
//
//     A'_e = A_{2e} - U_{2e+1}^T U_{2e+1} - V_{2e-1}^T V_{2e-1}
//     S'[e+1, e] = -V_{2e+1}^T U_{2e+1}
//
// go to the next level's storage.  Solve: z_k = L_k^-1 r_k, r'_e = r_{2e} -
// U_{2e+1}^T z_{2e+1} - V_{2e-1}^T z_{2e-1} down the levels, y_k = L_k^-T (z_k
// - U_k y_{k-1} - V_k y_{k+1}) back up.
//
// Kernels.  opty_normal_blocks: one workgroup per constraint node, the
// node's block of the Jacobian (trajectory columns in ascending (row, off)
// order, a pruned entry 0) in LDS; an element is one chain of fma over the
// columns in that order.  opty_normal_elim: one workgroup per eliminated row,
// A_k and its two couplings in LDS.  opty_normal_update: one workgroup per
// surviving row.  opty_normal_fwd_elim / opty_normal_fwd_update /
// opty_normal_bwd: the same ownership for one right-hand side.  The owner of
// an element computes it in a fixed order and stores it once: no atomics on
// values, the same bits in every call and for both memory kinds.  A pivot
// that is not positive and finite is replaced by 1 and recorded -- the
// smallest (level, row) of the factorisation, by an unsigned minimum on one
// word of the handle --: a numerical status, nothing loops or traps.
#include "opty_internal.h"

#include <cmath>
#include <cstdint>
#include <map>

using namespace opty;

namespace {

constexpr int kThreads = 256;       // blocks, elim, update
constexpr int kSolveThreads = 128;  // the kernels of one right-hand side
constexpr unsigned long long kNoPivot = ~0ull;

// odd pitch in doubles: lanes that walk a column of a tile hit distinct banks
__host__ __device__ constexpr int pitch(int n) { return n | 1; }

struct BlocksArgs {
    const double *jac;          // the Jacobian's values
    const double *d;            // null: all ones
    double delta;
    double *A, *B;
    const int *ent;             // (equation, sorted column) -> entry or -1
    const long long *ebase;     // entry e of node i is jac[ebase[e] +
    const int *estride;         //                          i*estride[e]]
    const int *crow, *coff;     // (row, off) of sorted column c
    const int *b0, *b1, *brow;  // coupled row t: its offset-0 / offset-1
    long long N, ncn;           // ... sorted column, its free row
    int M, Ct, nb;
};

// LDS: G (M x Ct) | X0 (M x nb) | dk (Ct) | db (nb) | b1 (nb ints)
__host__ __device__ constexpr size_t blocks_lds(int M, int Ct, int nb) {
    return ((size_t)M*pitch(Ct) + (size_t)M*pitch(nb) + Ct + nb)*
               sizeof(double) + (size_t)(nb + 1)*sizeof(int);
}

__global__ void __launch_bounds__(kThreads)
opty_normal_blocks(BlocksArgs a) {
    extern __shared__ double lds[];
    const int M = a.M, Ct = a.Ct, nb = a.nb, pg = pitch(Ct), pb = pitch(nb);
    double *G = lds, *X0 = G + (size_t)M*pg, *dk = X0 + (size_t)M*pb,
           *db = dk + Ct;
    int *b1 = reinterpret_cast<int *>(db + nb);
    const long long i = blockIdx.x;
    const bool coupled = i + 1 < a.ncn;
    const int tid = threadIdx.x;
    for (int t = tid; t < M*Ct; t += kThreads) {
        const int r = t/Ct, c = t - r*Ct, e = a.ent[t];
        G[r*pg + c] = e >= 0 ? a.jac[a.ebase[e] + i*a.estride[e]] : 0.0;
    }
    for (int t = tid; t < Ct; t += kThreads)
        dk[t] = a.d ? a.d[(long long)a.crow[t]*a.N + i + a.coff[t]] : 1.0;
    if (coupled) {
        for (int t = tid; t < M*nb; t += kThreads) {
            const int r = t/nb, c = t - r*nb, e = a.ent[r*Ct + a.b0[c]];
            X0[r*pb + c] =
                e >= 0 ? a.jac[a.ebase[e] + (i + 1)*a.estride[e]] : 0.0;
        }
        for (int t = tid; t < nb; t += kThreads) {
            db[t] = a.d ? a.d[(long long)a.brow[t]*a.N + i + 1] : 1.0;
            b1[t] = a.b1[t];
        }
    }
    __syncthreads();
    // the lower triangle; its mirror is the same chain with the factors of
    // every product swapped
    double *Ai = a.A + i*M*M;
    for (int t = tid; t < M*M; t += kThreads) {
        const int r = t/M, c = t - r*M;
        if (c > r) continue;
        double acc = 0.0;
        for (int k = 0; k < Ct; ++k)
            acc = fma(G[r*pg + k], G[c*pg + k]/dk[k], acc);
        if (r == c) {
            Ai[t] = acc + a.delta;
        } else {
            Ai[t] = acc;
            Ai[c*M + r] = acc;
        }
    }
    if (coupled) {
        double *Bi = a.B + i*M*M;
        for (int t = tid; t < M*M; t += kThreads) {
            const int r = t/M, c = t - r*M;
            double acc = 0.0;
            for (int k = 0; k < nb; ++k)
                acc = fma(X0[r*pb + k], G[c*pg + b1[k]]/db[k], acc);
            Bi[t] = acc;
        }
    }
}

// LDS of opty_normal_elim / opty_normal_update: three tiles
__host__ __device__ constexpr size_t tiles_lds(int M) {
    return (size_t)3*M*pitch(M)*sizeof(double);
}

struct ElimArgs {
    double *A, *B;              // the level's blocks (in place)
    long long n;                // its rows
    unsigned long long *flag;
    unsigned long long key;     // (level << 40) | 0: + row = the pivot's key
    int M, single;              // single: the level has one row
};

__global__ void __launch_bounds__(kThreads)
opty_normal_elim(ElimArgs a) {
    extern __shared__ double lds[];
    const int M = a.M, p = pitch(M), tid = threadIdx.x;
    double *L = lds, *U = L + (size_t)M*p, *V = U + (size_t)M*p;
    const long long k = a.single ? 0 : 2*(long long)blockIdx.x + 1;
    const bool hasU = !a.single, hasV = !a.single && k + 1 < a.n;
    double *Ak = a.A + k*M*M;
    double *Uk = hasU ? a.B + (k - 1)*M*M : nullptr;    // S[k, k-1]
    double *Vk = hasV ? a.B + k*M*M : nullptr;          // S[k+1, k]
    for (int t = tid; t < M*M; t += kThreads) {
        const int r = t/M, c = t - r*M;
        L[r*p + c] = c <= r ? Ak[t] : 0.0;
        if (hasU) U[r*p + c] = Uk[t];
        if (hasV) V[c*p + r] = Vk[t];                   // S[k, k+1]
    }
    __syncthreads();
    for (int j = 0; j < M; ++j) {
        double pj = L[j*p + j];
        if (!(pj > 0.0) || !(pj < INFINITY)) {
            if (tid == 0) atomicMin(a.flag, a.key + (unsigned long long)k);
            pj = 1.0;
        }
        const double s = sqrt(pj);
        __syncthreads();
        for (int r = j + tid; r < M; r += kThreads)
            L[r*p + j] = r == j ? s : L[r*p + j]/s;
        __syncthreads();
        const int m = M - 1 - j;
        for (int t = tid; t < m*m; t += kThreads) {
            const int q = t/m, r = j + 1 + q, c = j + 1 + (t - q*m);
            if (c <= r)
                L[r*p + c] = fma(-L[r*p + j], L[c*p + j], L[r*p + c]);
        }
        __syncthreads();
    }
    // lane = column of U, then of V: forward substitution down the column
    for (int col = tid; col < 2*M; col += kThreads) {
        const bool second = col >= M;
        if (second ? !hasV : !hasU) continue;
        double *X = (second ? V : U) + (second ? col - M : col);
        for (int r = 0; r < M; ++r) {
            double x = X[r*p];
            for (int c = 0; c < r; ++c) x = fma(-L[r*p + c], X[c*p], x);
            X[r*p] = x/L[r*p + r];
        }
    }
    __syncthreads();
    for (int t = tid; t < M*M; t += kThreads) {
        const int r = t/M, c = t - r*M;
        Ak[t] = L[r*p + c];
        if (hasU) Uk[t] = U[r*p + c];
        if (hasV) Vk[t] = V[r*p + c];
    }
}

struct UpdateArgs {
    const double *A, *B;        // the level's factors
    double *An, *Bn;            // the next level's blocks
    long long n;                // rows of the level
    int M;
};

__global__ void __launch_bounds__(kThreads)
opty_normal_update(UpdateArgs a) {
    extern __shared__ double lds[];
    const int M = a.M, p = pitch(M), tid = threadIdx.x;
    double *UR = lds, *VL = UR + (size_t)M*p, *VR = VL + (size_t)M*p;
    const long long e = blockIdx.x, k = 2*e;
    const bool right = k + 1 < a.n, left = e > 0, next = k + 2 < a.n;
    const size_t MM = (size_t)M*M;
    for (int t = tid; t < M*M; t += kThreads) {
        const int r = t/M, c = t - r*M;
        if (right) UR[r*p + c] = a.B[k*MM + t];         // U_{2e+1}
        if (left) VL[r*p + c] = a.B[(k - 1)*MM + t];    // V_{2e-1}
        if (next) VR[r*p + c] = a.B[(k + 1)*MM + t];    // V_{2e+1}
    }
    __syncthreads();
    for (int t = tid; t < M*M; t += kThreads) {
        const int r = t/M, c = t - r*M;
        if (c <= r) {
            double acc = a.A[k*MM + t];
            if (right)
                for (int q = 0; q < M; ++q)
                    acc = fma(-UR[q*p + r], UR[q*p + c], acc);
            if (left)
                for (int q = 0; q < M; ++q)
                    acc = fma(-VL[q*p + r], VL[q*p + c], acc);
            a.An[e*MM + t] = acc;
            if (c < r) a.An[e*MM + (size_t)c*M + r] = acc;
        }
        if (next) {
            double acc = 0.0;
            for (int q = 0; q < M; ++q)
                acc = fma(-VR[q*p + r], UR[q*p + c], acc);
            a.Bn[e*MM + t] = acc;
        }
    }
}

// LDS of the kernels of one right-hand side: one tile and two vectors
__host__ __device__ constexpr size_t solve_lds(int M) {
    return ((size_t)M*pitch(M) + 2*(size_t)M)*sizeof(double);
}

struct SolveArgs {
    const double *A, *B;        // the level's factors
    const double *src;          // forward: the level's right-hand sides
    double *z;                  // ... its z (eliminated rows)
    double *dst;                // forward: the next level's right-hand sides;
    const double *up;           // backward: the next level's y
    long long n;                // rows of the level
    long long eq_stride;        // > 0: src (forward) / dst (backward) is the
    int M, single;              //   caller's vector, [j*eq_stride + row]
};

__device__ inline long long at(const SolveArgs &a, long long row, int j) {
    return a.eq_stride > 0 ? j*a.eq_stride + row : row*a.M + j;
}

// z_k = L_k^-1 r_k, one workgroup per eliminated row
__global__ void __launch_bounds__(kSolveThreads)
opty_normal_fwd_elim(SolveArgs a) {
    extern __shared__ double lds[];
    const int M = a.M, p = pitch(M), tid = threadIdx.x;
    double *L = lds, *x = L + (size_t)M*p;
    const long long k = a.single ? 0 : 2*(long long)blockIdx.x + 1;
    const double *Ak = a.A + k*M*M;
    for (int t = tid; t < M*M; t += kSolveThreads) {
        const int r = t/M, c = t - r*M;
        L[r*p + c] = Ak[t];
    }
    for (int j = tid; j < M; j += kSolveThreads) x[j] = a.src[at(a, k, j)];
    __syncthreads();
    for (int j = 0; j < M; ++j) {
        const double xj = x[j]/L[j*p + j];
        __syncthreads();
        if (tid == 0) x[j] = xj;
        for (int r = j + 1 + tid; r < M; r += kSolveThreads)
            x[r] = fma(-L[r*p + j], xj, x[r]);
        __syncthreads();
    }
    for (int j = tid; j < M; j += kSolveThreads) a.z[k*M + j] = x[j];
}

// r'_e = r_{2e} - U_{2e+1}^T z_{2e+1} - V_{2e-1}^T z_{2e-1}, one workgroup per
// surviving row; lane = element (the factors are read along their rows)
__global__ void __launch_bounds__(kSolveThreads)
opty_normal_fwd_update(SolveArgs a) {
    extern __shared__ double lds[];
    const int M = a.M, tid = threadIdx.x;
    double *zr = lds, *zl = lds + M;
    const long long e = blockIdx.x, k = 2*e;
    const bool right = k + 1 < a.n, left = e > 0;
    const size_t MM = (size_t)M*M;
    for (int j = tid; j < M; j += kSolveThreads) {
        zr[j] = right ? a.z[(k + 1)*M + j] : 0.0;
        zl[j] = left ? a.z[(k - 1)*M + j] : 0.0;
    }
    __syncthreads();
    for (int j = tid; j < M; j += kSolveThreads) {
        double acc = a.src[at(a, k, j)];
        if (right) {
            const double *U = a.B + k*MM;
            for (int q = 0; q < M; ++q) acc = fma(-U[q*M + j], zr[q], acc);
        }
        if (left) {
            const double *V = a.B + (k - 1)*MM;
            for (int q = 0; q < M; ++q) acc = fma(-V[q*M + j], zl[q], acc);
        }
        a.dst[e*M + j] = acc;
    }
}

// one workgroup per row of the level: a surviving row takes its y from the
// next level, an eliminated one is y_k = L_k^-T (z_k - U_k y_{k-1} - V_k
// y_{k+1})
__global__ void __launch_bounds__(kSolveThreads)
opty_normal_bwd(SolveArgs a) {
    extern __shared__ double lds[];
    const int M = a.M, p = pitch(M), tid = threadIdx.x;
    double *T = lds, *x = T + (size_t)M*p, *v = x + M;
    const long long k = blockIdx.x;
    const bool eliminated = a.single || (k & 1);
    if (!eliminated) {
        for (int j = tid; j < M; j += kSolveThreads)
            a.dst[at(a, k, j)] = a.up[(k/2)*M + j];
        return;
    }
    const size_t MM = (size_t)M*M;
    const bool hasU = !a.single, hasV = !a.single && k + 1 < a.n;
    for (int j = tid; j < M; j += kSolveThreads) x[j] = a.z[k*M + j];
    for (int pass = 0; pass < 2; ++pass) {
        if (pass == 0 ? !hasU : !hasV) continue;
        const double *X = a.B + (pass == 0 ? k - 1 : k)*MM;
        const double *y = a.up + (pass == 0 ? (k - 1)/2 : (k + 1)/2)*M;
        __syncthreads();
        for (int t = tid; t < M*M; t += kSolveThreads) {
            const int r = t/M, c = t - r*M;
            T[r*p + c] = X[t];
        }
        for (int j = tid; j < M; j += kSolveThreads) v[j] = y[j];
        __syncthreads();
        for (int r = tid; r < M; r += kSolveThreads) {
            double acc = x[r];
            for (int c = 0; c < M; ++c) acc = fma(-T[r*p + c], v[c], acc);
            x[r] = acc;
        }
    }
    __syncthreads();
    const double *Ak = a.A + k*MM;
    for (int t = tid; t < M*M; t += kSolveThreads) {
        const int r = t/M, c = t - r*M;
        T[r*p + c] = Ak[t];
    }
    __syncthreads();
    for (int j = M - 1; j >= 0; --j) {
        const double xj = x[j]/T[j*p + j];
        __syncthreads();
        if (tid == 0) x[j] = xj;
        for (int r = tid; r < j; r += kSolveThreads)
            x[r] = fma(-T[j*p + r], xj, x[r]);
        __syncthreads();
    }
    for (int j = tid; j < M; j += kSolveThreads) a.dst[at(a, k, j)] = x[j];
}

// where wrt column k of the block lives in `free` (column_side of
// codegen/program.py)
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

bool overlaps(const double *a, size_t na, const double *b, size_t nb) {
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a0 < b0 + nb*sizeof(double) && b0 < a0 + na*sizeof(double);
}

// the largest M whose three tiles fit `limit` bytes of LDS
int largest_m(size_t limit) {
    int M = 0;
    while (tiles_lds(M + 1) <= limit) ++M;
    return M;
}

struct Level {
    long long n = 0;
    double *A = nullptr, *B = nullptr, *r = nullptr, *z = nullptr,
           *y = nullptr;
};

enum { kNone = 0, kEnqueued = 1, kFactored = 2, kFailed = 3 };

}  // namespace

struct opty_hip_normal : Borrowed {
    int M = 0, P = 0, Ct = 0, nb = 0;
    long long N = 0, ncn = 0;
    size_t njac = 0, nd = 0;            // values read of jac_values and of d
    size_t table_bytes = 0, level_doubles = 0;
    std::vector<Level> levels;
    int state = kNone;
    int32_t fail_level = -1;
    int64_t fail_row = -1;
    int *d_ent = nullptr, *d_estride = nullptr, *d_crow = nullptr,
        *d_coff = nullptr, *d_b0 = nullptr, *d_b1 = nullptr,
        *d_brow = nullptr;
    long long *d_ebase = nullptr;
    unsigned long long *d_flag = nullptr;
    double *d_ws = nullptr;             // every level's storage
    // staging for host callers
    double *d_jval = nullptr, *d_dval = nullptr, *d_A = nullptr,
           *d_B = nullptr, *d_r = nullptr, *d_y = nullptr;
    size_t mrows() const { return (size_t)M*(size_t)ncn; }
};

namespace {

int check_delta(double delta_c) {
    if (!(delta_c >= 0.0) || !(delta_c < INFINITY))
        return fail("delta_c %g is not a finite value >= 0", delta_c);
    return 0;
}

int launch_blocks(opty_hip_normal *h, const double *jac, const double *d,
                  double delta_c, double *A, double *B) {
    BlocksArgs a{};
    a.jac = jac;
    a.d = d;
    a.delta = delta_c;
    a.A = A;
    a.B = B;
    a.ent = h->d_ent;
    a.ebase = h->d_ebase;
    a.estride = h->d_estride;
    a.crow = h->d_crow;
    a.coff = h->d_coff;
    a.b0 = h->d_b0;
    a.b1 = h->d_b1;
    a.brow = h->d_brow;
    a.N = h->N;
    a.ncn = h->ncn;
    a.M = h->M;
    a.Ct = h->Ct;
    a.nb = h->nb;
    hipLaunchKernelGGL(opty_normal_blocks, dim3((unsigned)h->ncn),
                       dim3(kThreads), blocks_lds(h->M, h->Ct, h->nb),
                       h->stream, a);
    HIP_TRY(hipGetLastError());
    return 0;
}

// the status of the last factorisation, waited for once
int resolve(opty_hip_normal *h) {
    if (h->state != kEnqueued) return 0;
    unsigned long long flag = 0;
    HIP_TRY(hipMemcpyAsync(&flag, h->d_flag, sizeof flag,
                           hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(sync_target(h->stream)));
    if (flag == kNoPivot) {
        h->state = kFactored;
        h->fail_level = -1;
        h->fail_row = -1;
    } else {
        h->state = kFailed;
        h->fail_level = (int32_t)(flag >> 40);
        h->fail_row = (int64_t)(flag & ((1ull << 40) - 1));
    }
    return 0;
}

}  // namespace

extern "C" {

int opty_hip_normal_create(opty_hip_problem *p,
                           const opty_hip_normal_desc *desc,
                           opty_hip_normal **out) {
    if (!p || !desc || !out) return fail("null argument");
    const int M = desc->M, P = desc->P;
    if (M < 1 || P < 0)
        return fail("bad normal-matrix descriptor (M %d, P %d)", M, P);
    if (desc->layout != OPTY_HIP_LAYOUT_COO &&
        desc->layout != OPTY_HIP_LAYOUT_CSR)
        return fail("the normal matrix takes the Jacobian in "
                    "OPTY_HIP_LAYOUT_COO or OPTY_HIP_LAYOUT_CSR, not layout "
                    "%d", desc->layout);
    if (P > 0 && !desc->pattern) return fail("null block pattern");
    if (p->d.N < 2) return fail("N %lld < 2", (long long)p->d.N);
    const long long N = p->d.N, ncn = N - 1;
    if (ncn >= (1ll << 31))
        return fail("%lld constraint nodes, the limit is 2^31 - 1", ncn);
    const bool csr = desc->layout == OPTY_HIP_LAYOUT_CSR;
    // entries, their position rule and the trajectory columns they touch
    std::map<std::pair<int, int>, int> cols;        // (row, off) -> sorted
    std::vector<std::pair<int, int>> side((size_t)P);
    std::vector<int> eS(M, 0), eL(M, 0);
    for (int e = 0; e < P; ++e) {
        const int j = desc->pattern[2*e], k = desc->pattern[2*e + 1];
        if (j < 0 || j >= M || k < 0 || k >= p->d.C)
            return fail("block pattern entry %d: (%d, %d) outside %d x %d",
                        e, j, k, M, p->d.C);
        if (csr && e > 0 && j < desc->pattern[2*(e - 1)])
            return fail("block pattern entry %d: the entries of the CSR "
                        "layout are not grouped by equation, ascending", e);
        if (eL[j]++ == 0) eS[j] = e;
        side[e] = column_side(p->d, k);
        if (side[e].first >= 0) cols[side[e]] = 0;
    }
    const int Ct = (int)cols.size();
    std::vector<int> crow, coff;
    for (auto &kv : cols) {
        kv.second = (int)crow.size();
        crow.push_back(kv.first.first);
        coff.push_back(kv.first.second);
    }
    std::vector<int> ent((size_t)M*std::max(1, Ct), -1), estride((size_t)P);
    std::vector<long long> ebase((size_t)P);
    for (int e = 0; e < P; ++e) {
        const int j = desc->pattern[2*e];
        ebase[e] = csr ? (long long)eS[j]*ncn + (e - eS[j]) : e;
        estride[e] = csr ? eL[j] : P;
        if (side[e].first < 0) continue;            // a tail column
        int &slot = ent[(size_t)j*Ct + cols[side[e]]];
        if (slot >= 0)
            return fail("block pattern entry %d repeats entry %d: (%d, %d)",
                        e, slot, j, desc->pattern[2*e + 1]);
        slot = e;
    }
    // free rows with an offset-0 and an offset-1 column
    std::vector<int> b0, b1, brow;
    for (auto &kv : cols)
        if (kv.first.second == 0) {
            auto other = cols.find({kv.first.first, 1});
            if (other == cols.end()) continue;
            b0.push_back(kv.second);
            b1.push_back(other->second);
            brow.push_back(kv.first.first);
        }
    const int nb = (int)b0.size();

    if (int rc = use_device(p)) return rc;
    int limit = 0;
    HIP_TRY(hipDeviceGetAttribute(&limit,
                                  hipDeviceAttributeMaxSharedMemoryPerBlock,
                                  p->d.device));
    if (tiles_lds(M) > (size_t)limit)
        return fail("%d equations need %zu bytes of LDS per block (three "
                    "tiles of %d x %d doubles), the limit is %d bytes (%d "
                    "equations)", M, tiles_lds(M), M, pitch(M), limit,
                    largest_m((size_t)limit));
    if (blocks_lds(M, Ct, nb) > (size_t)limit)
        return fail("%d equations over %d trajectory columns need %zu bytes "
                    "of LDS per block, the limit is %d bytes", M, Ct,
                    blocks_lds(M, Ct, nb), limit);
    // more than 64 KiB of dynamic LDS has to be asked for
    if (tiles_lds(M) > 65536) {
        HIP_TRY(hipFuncSetAttribute(
            (const void *)opty_normal_elim,
            hipFuncAttributeMaxDynamicSharedMemorySize, (int)limit));
        HIP_TRY(hipFuncSetAttribute(
            (const void *)opty_normal_update,
            hipFuncAttributeMaxDynamicSharedMemorySize, (int)limit));
    }
    if (blocks_lds(M, Ct, nb) > 65536)
        HIP_TRY(hipFuncSetAttribute(
            (const void *)opty_normal_blocks,
            hipFuncAttributeMaxDynamicSharedMemorySize, (int)limit));

    auto *h = new opty_hip_normal;
    h->p = p;
    h->device = p->d.device;
    h->M = M;
    h->P = P;
    h->Ct = Ct;
    h->nb = nb;
    h->N = N;
    h->ncn = ncn;
    h->njac = (size_t)P*(size_t)ncn;
    h->nd = (size_t)(p->d.n + p->d.q)*(size_t)N;
    auto refuse = [&](int rc) {
        (void)opty_hip_normal_destroy(h);
        return rc;
    };
    // every entry of every node stays inside the values that are read
    for (int e = 0; e < P; ++e)
        if (ebase[e] < 0 ||
            ebase[e] + (ncn - 1)*estride[e] >= (long long)h->njac)
            return refuse(fail("block pattern entry %d leaves the %zu values "
                               "of the Jacobian's blocks", e, h->njac));
    const size_t MM = (size_t)M*M;
    size_t total = 0;
    for (long long n = ncn;; n = (n + 1)/2) {
        Level lv;
        lv.n = n;
        h->levels.push_back(lv);
        total += (size_t)n*MM + (size_t)(n - 1)*MM + 3*(size_t)n*M;
        if (n == 1) break;
    }
    h->level_doubles = total;
    auto device_side = [&]() -> int {
        if (int rc = upload(&h->d_ent, ent.data(), ent.size())) return rc;
        if (int rc = upload(&h->d_ebase, ebase.data(), ebase.size()))
            return rc;
        if (int rc = upload(&h->d_estride, estride.data(), estride.size()))
            return rc;
        if (int rc = upload(&h->d_crow, crow.data(), crow.size())) return rc;
        if (int rc = upload(&h->d_coff, coff.data(), coff.size())) return rc;
        if (int rc = upload(&h->d_b0, b0.data(), b0.size())) return rc;
        if (int rc = upload(&h->d_b1, b1.data(), b1.size())) return rc;
        if (int rc = upload(&h->d_brow, brow.data(), brow.size())) return rc;
        if (int rc = ensure(&h->d_flag, 1)) return rc;
        return ensure(&h->d_ws, total);
    };
    if (int rc = device_side()) return refuse(rc);
    h->table_bytes = ent.size()*sizeof(int) + ebase.size()*sizeof(long long) +
        (estride.size() + crow.size() + coff.size() + b0.size() + b1.size() +
         brow.size())*sizeof(int) + sizeof(unsigned long long);
    double *at = h->d_ws;
    for (Level &lv : h->levels) {
        lv.A = at;
        at += (size_t)lv.n*MM;
        lv.B = at;
        at += (size_t)(lv.n - 1)*MM;
        lv.r = at;
        at += (size_t)lv.n*M;
        lv.z = at;
        at += (size_t)lv.n*M;
        lv.y = at;
        at += (size_t)lv.n*M;
    }
    *out = h;
    return 0;
}

int opty_hip_normal_destroy(opty_hip_normal *h) {
    if (!h) return 0;
    borrowed_destroy(h, {h->d_ent, h->d_ebase, h->d_estride, h->d_crow,
                         h->d_coff, h->d_b0, h->d_b1, h->d_brow, h->d_flag,
                         h->d_ws, h->d_jval, h->d_dval, h->d_A, h->d_B,
                         h->d_r, h->d_y});
    delete h;
    return 0;
}

int64_t opty_hip_normal_workspace_bytes(const opty_hip_normal *h) {
    return h ? (int64_t)(h->level_doubles*sizeof(double) + h->table_bytes)
             : -1;
}

int32_t opty_hip_normal_max_equations(const opty_hip_normal *h) {
    if (!h) return -1;
    int limit = 0;
    if (hipDeviceGetAttribute(&limit,
                              hipDeviceAttributeMaxSharedMemoryPerBlock,
                              h->device) != hipSuccess) {
        (void)hipGetLastError();
        return -1;
    }
    return largest_m((size_t)limit);
}

int opty_hip_normal_blocks(opty_hip_normal *h, const double *jac_values,
                           const double *d, double delta_c, double *A,
                           double *B, int32_t mem) {
    if (!h || !jac_values || !A) return fail("null argument");
    const size_t MM = (size_t)h->M*h->M, nA = (size_t)h->ncn*MM,
                 nB = (size_t)(h->ncn - 1)*MM;
    if (nB > 0 && !B) return fail("null argument");
    if (int rc = check_delta(delta_c)) return rc;
    for (auto in : {std::make_pair(jac_values, h->njac),
                    std::make_pair(d, d ? h->nd : (size_t)0)}) {
        if (!in.first) continue;
        if (overlaps(A, nA, in.first, in.second) ||
            (nB > 0 && overlaps(B, nB, in.first, in.second)))
            return fail("A or B overlaps an input");
    }
    if (nB > 0 && overlaps(A, nA, B, nB)) return fail("A overlaps B");
    if (int rc = borrowed_begin(h, mem, false)) return rc;
    double *dA = A, *dB = B;
    if (mem == OPTY_HIP_HOST) {
        if (int rc = stage_in(h, &jac_values, &h->d_jval, h->njac,
                              std::max<size_t>(1, h->njac)))
            return rc;
        if (d)
            if (int rc = stage_in(h, &d, &h->d_dval, h->nd,
                                  std::max<size_t>(1, h->nd)))
                return rc;
        if (int rc = ensure(&h->d_A, nA)) return rc;
        if (int rc = ensure(&h->d_B, nB)) return rc;
        dA = h->d_A;
        dB = h->d_B;
    }
    if (int rc = launch_blocks(h, jac_values, d, delta_c, dA, dB)) return rc;
    if (mem == OPTY_HIP_HOST) {
        if (int rc = stage_out(h, A, dA, nA*sizeof(double))) return rc;
        if (int rc = stage_out(h, B, dB, nB*sizeof(double))) return rc;
        return host_done(h);
    }
    return 0;
}

int opty_hip_normal_factor(opty_hip_normal *h, const double *jac_values,
                           const double *d, double delta_c, int32_t mem) {
    if (!h || !jac_values) return fail("null argument");
    if (int rc = check_delta(delta_c)) return rc;
    if (int rc = borrowed_begin(h, mem, false)) return rc;
    if (mem == OPTY_HIP_HOST) {
        if (int rc = stage_in(h, &jac_values, &h->d_jval, h->njac,
                              std::max<size_t>(1, h->njac)))
            return rc;
        if (d)
            if (int rc = stage_in(h, &d, &h->d_dval, h->nd,
                                  std::max<size_t>(1, h->nd)))
                return rc;
    }
    h->state = kNone;
    HIP_TRY(hipMemsetAsync(h->d_flag, 0xFF, sizeof(unsigned long long),
                           h->stream));
    if (int rc = launch_blocks(h, jac_values, d, delta_c, h->levels[0].A,
                               h->levels[0].B))
        return rc;
    const size_t lds = tiles_lds(h->M);
    for (size_t l = 0; l < h->levels.size(); ++l) {
        const Level &lv = h->levels[l];
        ElimArgs e{};
        e.A = lv.A;
        e.B = lv.B;
        e.n = lv.n;
        e.flag = h->d_flag;
        e.key = (unsigned long long)l << 40;
        e.M = h->M;
        e.single = lv.n == 1;
        const long long grid = lv.n == 1 ? 1 : lv.n/2;
        hipLaunchKernelGGL(opty_normal_elim, dim3((unsigned)grid),
                           dim3(kThreads), lds, h->stream, e);
        HIP_TRY(hipGetLastError());
        if (lv.n == 1) break;
        const Level &nx = h->levels[l + 1];
        UpdateArgs u{};
        u.A = lv.A;
        u.B = lv.B;
        u.An = nx.A;
        u.Bn = nx.B;
        u.n = lv.n;
        u.M = h->M;
        hipLaunchKernelGGL(opty_normal_update, dim3((unsigned)nx.n),
                           dim3(kThreads), lds, h->stream, u);
        HIP_TRY(hipGetLastError());
    }
    h->state = kEnqueued;
    if (mem == OPTY_HIP_HOST) return resolve(h);
    return 0;
}

int opty_hip_normal_factor_status(opty_hip_normal *h, int32_t *level,
                                  int64_t *row) {
    if (!h || !level || !row) return fail("null argument");
    if (h->state == kNone)
        return fail("no factorisation: opty_hip_normal_factor was never "
                    "called or did not succeed");
    if (int rc = use_device(h->p)) return rc;
    if (int rc = resolve(h)) return rc;
    *level = h->fail_level;
    *row = h->fail_row;
    return 0;
}

int opty_hip_normal_solve(opty_hip_normal *h, const double *r, double *y,
                          int32_t ncols, int64_t ld, int32_t mem) {
    if (!h || !r || !y) return fail("null argument");
    if (mem != OPTY_HIP_HOST && mem != OPTY_HIP_DEVICE)
        return fail("bad memory kind %d", mem);
    const size_t m = h->mrows();
    if (ncols < 0) return fail("ncols %d < 0", ncols);
    if (ld < (int64_t)m)
        return fail("ld %lld is less than the %zu rows of the normal matrix",
                    (long long)ld, m);
    if (ncols > 0) {
        const size_t span = (size_t)(ncols - 1)*(size_t)ld + m;
        if (overlaps(y, span, r, span)) return fail("y overlaps r");
    }
    if (h->state == kNone)
        return fail("solve before a successful factorisation "
                    "(opty_hip_normal_factor)");
    if (int rc = use_device(h->p)) return rc;
    if (int rc = resolve(h)) return rc;
    if (h->state != kFactored)
        return fail("solve before a successful factorisation: the last one "
                    "met a pivot that is not positive and finite at level "
                    "%d, row %lld", h->fail_level, (long long)h->fail_row);
    if (int rc = borrowed_begin(h, mem, false)) return rc;
    const size_t lds = solve_lds(h->M);
    const size_t nlev = h->levels.size();
    for (int32_t col = 0; col < ncols; ++col) {
        const double *rc_ = r + (size_t)col*(size_t)ld;
        double *yc = y + (size_t)col*(size_t)ld;
        if (mem == OPTY_HIP_HOST) {
            if (int rc = stage_in(h, &rc_, &h->d_r, m, m)) return rc;
            if (int rc = ensure(&h->d_y, m)) return rc;
        }
        double *yd = mem == OPTY_HIP_HOST ? h->d_y : yc;
        for (size_t l = 0; l < nlev; ++l) {
            const Level &lv = h->levels[l];
            SolveArgs a{};
            a.A = lv.A;
            a.B = lv.B;
            a.src = l == 0 ? rc_ : lv.r;
            a.z = lv.z;
            a.n = lv.n;
            a.eq_stride = l == 0 ? h->ncn : 0;
            a.M = h->M;
            a.single = lv.n == 1;
            const long long grid = lv.n == 1 ? 1 : lv.n/2;
            hipLaunchKernelGGL(opty_normal_fwd_elim, dim3((unsigned)grid),
                               dim3(kSolveThreads), lds, h->stream, a);
            HIP_TRY(hipGetLastError());
            if (lv.n == 1) break;
            a.dst = h->levels[l + 1].r;
            hipLaunchKernelGGL(opty_normal_fwd_update,
                               dim3((unsigned)h->levels[l + 1].n),
                               dim3(kSolveThreads), lds, h->stream, a);
            HIP_TRY(hipGetLastError());
        }
        for (size_t l = nlev; l-- > 0;) {
            const Level &lv = h->levels[l];
            SolveArgs a{};
            a.A = lv.A;
            a.B = lv.B;
            a.z = lv.z;
            a.dst = l == 0 ? yd : lv.y;
            a.up = l + 1 < nlev ? h->levels[l + 1].y : nullptr;
            a.n = lv.n;
            a.eq_stride = l == 0 ? h->ncn : 0;
            a.M = h->M;
            a.single = lv.n == 1;
            hipLaunchKernelGGL(opty_normal_bwd, dim3((unsigned)lv.n),
                               dim3(kSolveThreads), lds, h->stream, a);
            HIP_TRY(hipGetLastError());
        }
        if (mem == OPTY_HIP_HOST)
            if (int rc = stage_out(h, yc, h->d_y, m*sizeof(double)))
                return rc;
    }
    if (mem == OPTY_HIP_HOST) return host_done(h);
    return 0;
}

}  // extern "C"
