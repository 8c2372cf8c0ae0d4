// hessmv.cpp -- the Hessian-product handle of libopty_hip.so: y = H v from the
// stored triplets of the Hessian of the Lagrangian (include/opty_hip.h,
// "Hessian operator").  H is the symmetric matrix whose lower triangle is the
// SUM of the triplets; the value vector is laid out as Problem.hessian returns
// it: [node section | instance entries | objective section | parameter-
// parameter entries].
//
// The handle borrows its problem handle for N, n, q, r, s, device and stream.
// It loads no code object: the two kernels below are part of this library and
// serve every problem.  Both node-indexed sections have closed-form indices:
// relative to node i every side of an entry is (row, slot) -- free index
// row*N + i + slot, slot in {0, 1} -- or a tail entry.  The distinct sides get
// one slot each in a small table (trajectory sides first, then tail sides);
// opty_hessmv walks the entries once per block and adds value * v[other side]
// into the lane's column of an LDS accumulator acc[side][lane].
//
//   y[R*N + p]  = S_R0(node p) + S_R1(node p - 1)      (trajectory row R)
//   y[tail + j] = sum over all nodes of S_tail_j       (parameter / h)
//
// Blocks of 64 lanes advance by 63 nodes (opty_vjp's scheme): lane l of block
// b is node 63 b + l, lane l >= 1 writes p = 63 b + l from its own S_R0 and
// lane l - 1's S_R1, read from LDS; lane 0 of block 0 writes p = 0.  Lane 0 of
// a later block repeats the previous block's last node and counts as zero in
// the tail sums.  Every element of y is stored once; no atomics.
//
// A window [wa, wb) of the constraint nodes (opty_hip_hessmv_apply_shard): the
// same lanes from the GLOBAL v at the global node index.  Block B starts at
// node wa - (wa > 0) + 63 B -- a window that does not start the problem begins
// one (halo) node early, whose S_R1 the first owned time node needs --, stores
// the time nodes p in [wa, pend), pend = wb + (wb == N - 1), at y[R*ostride +
// p - wa], and its tail partials cover the nodes [wa, wb).  The window is
// wave-uniform; the whole problem is the window [0, N - 1) with ostride = N.
//
// Block products Y = H V (opty_hip_hessmv_apply_block): opty_hessmv_block<K>
// keeps K columns in flight -- K values of v and K accumulators per side and
// lane -- so that a value goes through the tile once for all K; per column the
// operations and their order are opty_hessmv's, so column c has the bits of
// opty_hip_hessmv_apply on column c alone.
#include "opty_internal.h"

#include <cstdint>
#include <map>

using namespace opty;

namespace {

constexpr long long kStride = 63;   // nodes a block advances by
constexpr int kChunk = 32;          // entries of a node per LDS tile
// odd pitch in doubles: the 32 lanes of a half wave that read one column of
// the tile with 8-byte reads hit 32 distinct pairs of the 64 banks
constexpr int kPitch = kChunk + 1;
constexpr size_t kTileBytes = (size_t)64*kPitch*sizeof(double);

struct MvArgs {
    const double *val;      // node section, val[i*PH + e]
    const double *oval;     // objective section, oval[e*ncn + j]
    const double *v;
    double *y;
    double *part;           // part[b*nT + t]
    const int *ent;         // (side a, side b) per node entry
    const int *oent;        // ... per objective entry
    const int *sides;       // (row, slot) per side; row -1: (-1, tail offset)
    const int *rowside;     // side of (R, 0) and (R, 1) per trajectory row, or -1
    long long N;
    // the window: constraint nodes [wa, wb), owned time nodes [wa, pend); val
    // starts at node wa - (wa > 0), y at time node wa, rows ostride apart
    long long wa, wb, pend, ostride;
    int PH, E, nS, nT, nrows;
};

// lane = constraint node (= quadrature point); one wave per block
__global__ void __launch_bounds__(64)
opty_hessmv(MvArgs a) {
    extern __shared__ double lds[];
    const int lane = threadIdx.x;
    const int nA = a.nS + a.nT;
    double *tile = lds;                       // [64][kPitch]
    double *vs = lds + 64*kPitch;             // [nA][64]
    double *acc = vs + (size_t)nA*64;         // [nA][64]
    const long long N = a.N, ncn = N - 1;
    const long long lo = a.wa - (a.wa > 0 ? 1 : 0);
    const long long i0 = lo + (long long)blockIdx.x*kStride;
    const long long i = i0 + lane;
    const bool valid = i < a.wb;
    const long long tail = (long long)a.nrows*N;
    // nodes of this block that exist (>= 1: i0 < wb for every block)
    const int nv = (int)(a.wb - i0 < 64 ? a.wb - i0 : 64);
    // lane 0 is the halo node, or repeats the previous block's last node
    const bool first = lane > 0 || (blockIdx.x == 0 && a.wa == 0);

    // v at every side (a coalesced row load; tail sides broadcast), zero
    // accumulators.  i < wb <= ncn: row*N + i + slot <= row*N + N - 1.
    for (int s = 0; s < nA; ++s) {
        const int row = a.sides[2*s], off = a.sides[2*s + 1];
        double x = 0.0;
        if (valid) x = row >= 0 ? a.v[(long long)row*N + i + off]
                                : a.v[tail + off];
        vs[s*64 + lane] = x;
        acc[s*64 + lane] = 0.0;
    }

    // node section: the block's nv*PH values are contiguous; a chunk is kChunk
    // entries of every node, loaded as rows of w consecutive doubles (two
    // nodes per wave instruction), read back lane = node
    const double *blk = a.val + (i0 - lo)*a.PH;
    const int half = lane >> 5, col = lane & 31;
    for (int c0 = 0; c0 < a.PH; c0 += kChunk) {
        const int w = a.PH - c0 < kChunk ? a.PH - c0 : kChunk;
        __syncthreads();
        if (col < w)
            for (int nd = half; nd < nv; nd += 2)
                tile[nd*kPitch + col] = blk[(long long)nd*a.PH + c0 + col];
        __syncthreads();
        for (int k = 0; k < w; ++k) {
            const int sa = a.ent[2*(c0 + k)], sb = a.ent[2*(c0 + k) + 1];
            const double x = valid ? tile[lane*kPitch + k] : 0.0;
            acc[sa*64 + lane] += x*vs[sb*64 + lane];
            if (sa != sb) acc[sb*64 + lane] += x*vs[sa*64 + lane];
        }
    }

    // objective section: entry-major, lane = point, coalesced as it is
    for (int e = 0; e < a.E; ++e) {
        const int sa = a.oent[2*e], sb = a.oent[2*e + 1];
        const double x = valid ? a.oval[(long long)e*ncn + i] : 0.0;
        acc[sa*64 + lane] += x*vs[sb*64 + lane];
        if (sa != sb) acc[sb*64 + lane] += x*vs[sa*64 + lane];
    }
    __syncthreads();

    // trajectory rows: p = i; S_R0 of this lane + S_R1 of the lane before
    const bool writes = first && i < a.pend;
    for (int R = 0; R < a.nrows; ++R) {
        const int s0 = a.rowside[2*R], s1 = a.rowside[2*R + 1];
        double x = 0.0;
        if (s0 >= 0) x = acc[s0*64 + lane];
        if (s1 >= 0 && lane > 0) x += acc[s1*64 + lane - 1];
        if (writes) a.y[(long long)R*a.ostride + (i - a.wa)] = x;
    }

    // tail sides: a fixed tree over the lanes; the halo node is another
    // window's and the repeated node counts once
    for (int t = 0; t < a.nT; ++t) {
        double x = acc[(a.nS + t)*64 + lane];
        if (!first) x = 0.0;
        for (int d = 32; d >= 1; d >>= 1) x += __shfl_down(x, d);
        if (lane == 0) a.part[(long long)blockIdx.x*a.nT + t] = x;
    }
}

struct FinArgs {
    const double *part;
    const double *ival;     // instance values, then (pval) parameter-parameter
    const double *pval;
    const double *v;
    double *y;
    double *tail_part;      // ntail doubles, by tail offset
    const int *sides;
    const long long *irows, *icols, *prows, *pcols;
    long long nblk, tail;
    // the window (MvArgs); owner: this call adds the explicit triplets' tail
    // sides.  opty_hessmv_block_fin serves the whole problem only.
    long long N, wa, pend, ostride;
    int nS, nT, ntail, nnz_inst, T, owner;
};

// One wave, enqueued behind opty_hessmv: the tail entries (the window's block
// partials added in block order; an entry without a side is 0.0), then one
// lane applies the explicit triplets in stored order -- to the tail entries
// in LDS when the call owns the tail, to the trajectory entries the window
// owns (which opty_hessmv stored) in place; every other side is another
// window's.
__global__ void __launch_bounds__(64)
opty_hessmv_fin(FinArgs a) {
    extern __shared__ double tl[];          // [ntail]
    const int lane = threadIdx.x;
    for (int j = lane; j < a.ntail; j += 64) tl[j] = 0.0;
    __syncthreads();
    for (int t = lane; t < a.nT; t += 64) {
        double x = 0.0;
        for (long long b = 0; b < a.nblk; ++b) x += a.part[b*a.nT + t];
        tl[a.sides[2*(a.nS + t) + 1]] = x;
    }
    __syncthreads();
    if (lane == 0) {
        // (the whole problem: y[R*N + p] without the division)
        const bool whole = a.wa == 0 && a.pend == a.N && a.ostride == a.N;
        auto add = [&](long long at, double x) {
            if (at >= a.tail) {
                if (a.owner) tl[at - a.tail] += x;
            } else if (whole) {
                a.y[at] += x;
            } else {
                const long long R = at/a.N, p = at - R*a.N;
                if (p >= a.wa && p < a.pend)
                    a.y[R*a.ostride + (p - a.wa)] += x;
            }
        };
        auto apply = [&](long long r, long long c, double x) {
            add(r, x*a.v[c]);
            if (r != c) add(c, x*a.v[r]);
        };
        for (int k = 0; k < a.nnz_inst; ++k)
            apply(a.irows[k], a.icols[k], a.ival[k]);
        for (int k = 0; k < a.T; ++k)
            apply(a.prows[k], a.pcols[k], a.pval[k]);
    }
    __syncthreads();
    for (int j = lane; j < a.ntail; j += 64) a.tail_part[j] = tl[j];
}

// ---- K columns per pass ------------------------------------------------------
struct MvBlockArgs {
    MvArgs m;               // v, y: column 0; part[(c*gridDim.x + b)*nT + t]
    long long ldv, ldy;     // doubles between two columns of V / of Y
};

// opty_hessmv for K columns: vs and acc are [side][column][lane].  A value is
// read from the tile (or from memory, objective section) once; both of its
// side updates are then applied column by column.  Per column: opty_hessmv's
// operations in opty_hessmv's order, the multiply-add pinned to the fused form
// that opty_hessmv's `acc += x*v` is contracted to.
template <int K>
__global__ void __launch_bounds__(64)
opty_hessmv_block(MvBlockArgs b) {
    extern __shared__ double lds[];
    const MvArgs &a = b.m;
    const int lane = threadIdx.x;
    const int nA = a.nS + a.nT;
    double *tile = lds;                       // [64][kPitch]
    double *vs = lds + 64*kPitch;             // [nA][K][64]
    double *acc = vs + (size_t)nA*K*64;       // [nA][K][64]
    const long long N = a.N, ncn = N - 1;
    const long long i0 = (long long)blockIdx.x*kStride;
    const long long i = i0 + lane;
    const bool valid = i < ncn;
    const long long tail = (long long)a.nrows*N;
    const int nv = (int)(ncn - i0 < 64 ? ncn - i0 : 64);

    for (int s = 0; s < nA; ++s) {
        const int row = a.sides[2*s], off = a.sides[2*s + 1];
        const long long at = row >= 0 ? (long long)row*N + i + off
                                      : tail + off;
#pragma unroll
        for (int c = 0; c < K; ++c) {
            double x = 0.0;
            if (valid) x = a.v[c*b.ldv + at];
            vs[(s*K + c)*64 + lane] = x;
            acc[(s*K + c)*64 + lane] = 0.0;
        }
    }

    // one entry: value x on sides (sa, sb), every column
    auto entry = [&](int sa, int sb, double x) {
        double va[K], vb[K], t[K];
#pragma unroll
        for (int c = 0; c < K; ++c) {
            va[c] = vs[(sa*K + c)*64 + lane];
            vb[c] = vs[(sb*K + c)*64 + lane];
            t[c] = acc[(sa*K + c)*64 + lane];
        }
#pragma unroll
        for (int c = 0; c < K; ++c)
            acc[(sa*K + c)*64 + lane] = fma(x, vb[c], t[c]);
        if (sa != sb) {
#pragma unroll
            for (int c = 0; c < K; ++c) t[c] = acc[(sb*K + c)*64 + lane];
#pragma unroll
            for (int c = 0; c < K; ++c)
                acc[(sb*K + c)*64 + lane] = fma(x, va[c], t[c]);
        }
    };

    const double *blk = a.val + i0*a.PH;
    const int half = lane >> 5, col = lane & 31;
    for (int c0 = 0; c0 < a.PH; c0 += kChunk) {
        const int w = a.PH - c0 < kChunk ? a.PH - c0 : kChunk;
        __syncthreads();
        if (col < w)
            for (int nd = half; nd < nv; nd += 2)
                tile[nd*kPitch + col] = blk[(long long)nd*a.PH + c0 + col];
        __syncthreads();
        for (int k = 0; k < w; ++k)
            entry(a.ent[2*(c0 + k)], a.ent[2*(c0 + k) + 1],
                  valid ? tile[lane*kPitch + k] : 0.0);
    }

    for (int e = 0; e < a.E; ++e)
        entry(a.oent[2*e], a.oent[2*e + 1],
              valid ? a.oval[(long long)e*ncn + i] : 0.0);
    __syncthreads();

    const bool writes = (lane > 0 || blockIdx.x == 0) && i <= ncn;
    for (int R = 0; R < a.nrows; ++R) {
        const int s0 = a.rowside[2*R], s1 = a.rowside[2*R + 1];
#pragma unroll
        for (int c = 0; c < K; ++c) {
            double x = 0.0;
            if (s0 >= 0) x = acc[(s0*K + c)*64 + lane];
            if (s1 >= 0 && lane > 0) x += acc[(s1*K + c)*64 + lane - 1];
            if (writes) a.y[c*b.ldy + (long long)R*N + i] = x;
        }
    }

    for (int t = 0; t < a.nT; ++t)
#pragma unroll
        for (int c = 0; c < K; ++c) {
            double x = acc[((a.nS + t)*K + c)*64 + lane];
            if (lane == 0 && blockIdx.x > 0) x = 0.0;
            for (int d = 32; d >= 1; d >>= 1) x += __shfl_down(x, d);
            if (lane == 0)
                a.part[((long long)c*gridDim.x + blockIdx.x)*a.nT + t] = x;
        }
}

struct FinBlockArgs {
    FinArgs f;              // part, v, y: column 0
    long long ldv, ldy, ldpart;
};

// opty_hessmv_fin for the columns of a pass: block c is column c, with
// opty_hessmv_fin's operations in its order.
__global__ void __launch_bounds__(64)
opty_hessmv_block_fin(FinBlockArgs b) {
    extern __shared__ double tl[];          // [ntail]
    const FinArgs &a = b.f;
    const int lane = threadIdx.x;
    const double *part = a.part + blockIdx.x*b.ldpart;
    const double *v = a.v + blockIdx.x*b.ldv;
    double *y = a.y + blockIdx.x*b.ldy;
    for (int j = lane; j < a.ntail; j += 64) tl[j] = 0.0;
    __syncthreads();
    for (int t = lane; t < a.nT; t += 64) {
        double x = 0.0;
        for (long long k = 0; k < a.nblk; ++k) x += part[k*a.nT + t];
        tl[a.sides[2*(a.nS + t) + 1]] = x;
    }
    __syncthreads();
    if (lane == 0) {
        auto add = [&](long long at, double x) {
            if (at >= a.tail) tl[at - a.tail] += x;
            else y[at] += x;
        };
        auto apply = [&](long long r, long long c, double x) {
            add(r, x*v[c]);
            if (r != c) add(c, x*v[r]);
        };
        for (int k = 0; k < a.nnz_inst; ++k)
            apply(a.irows[k], a.icols[k], a.ival[k]);
        for (int k = 0; k < a.T; ++k)
            apply(a.prows[k], a.pcols[k], a.pval[k]);
    }
    __syncthreads();
    for (int j = lane; j < a.ntail; j += 64) y[a.tail + j] = tl[j];
}

constexpr int kMaxWidth = 4;        // widest instantiation of opty_hessmv_block

// LDS of one block of a pass over `width` columns
constexpr size_t lds_block(int sides, int width) {
    return kTileBytes + (size_t)sides*width*2*64*sizeof(double);
}

const void *block_kernel(int width) {
    switch (width) {
    case 2: return (const void *)opty_hessmv_block<2>;
    case 3: return (const void *)opty_hessmv_block<3>;
    case 4: return (const void *)opty_hessmv_block<4>;
    }
    return nullptr;
}

}  // namespace

struct opty_hip_hessmv : Borrowed {
    opty_hip_hessmv_desc d{};
    std::vector<int> sides;     // (row, slot) per side, trajectory sides first
    int nS = 0, nT = 0;
    int Kb = 1;                 // columns one pass of a block product takes
    size_t lds_main = 0, lds_fin = 0;
    int *d_ent = nullptr, *d_oent = nullptr, *d_sides = nullptr,
        *d_rowside = nullptr;
    long long *d_irows = nullptr, *d_icols = nullptr, *d_prows = nullptr,
              *d_pcols = nullptr;
    double *d_part = nullptr;
    // staging for host callers (v and y: cap_v / cap_y values, grown by a
    // block product to its columns)
    double *d_val = nullptr, *d_v = nullptr, *d_y = nullptr;
    size_t cap_v = 0, cap_y = 0;
    long long ncn() const { return p->d.N - 1; }
    long long blocks() const { return (ncn() + kStride - 1)/kStride; }
    // time nodes the non-empty window [wa, wb) owns end here
    long long pend(long long wb) const { return wb + (wb == ncn() ? 1 : 0); }
    // blocks of a non-empty window: block 0 of a window that starts the
    // problem stores 64 time nodes, every other block 63 (at most blocks())
    long long blocks(long long wa, long long wb) const {
        const long long todo = pend(wb) - wa - (wa == 0 ? 1 : 0);
        return std::max(1LL, (todo + kStride - 1)/kStride);
    }
    int nrows() const { return p->d.n + p->d.q; }
    int ntail() const { return p->d.r + p->d.s; }
    int64_t nnz() const {
        return (int64_t)(d.PH + d.E)*ncn() + d.nnz_inst + d.T;
    }
};

namespace {

// A staging vector of at least `count` values (a larger request replaces it:
// the host calls that use it have returned, so nothing reads it any more).
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

struct Pieces {
    const double *ival, *oval, *pval;
};

Pieces pieces(const opty_hip_hessmv *h, const double *values) {
    Pieces s;
    s.ival = values + (size_t)h->d.PH*h->ncn();
    s.oval = s.ival + h->d.nnz_inst;
    s.pval = s.oval + (size_t)h->d.E*h->ncn();
    return s;
}

MvArgs main_args(const opty_hip_hessmv *h, const double *values,
                 const double *v, double *out) {
    MvArgs a{};
    a.val = values;
    a.oval = pieces(h, values).oval;
    a.v = v;
    a.y = out;
    a.part = h->d_part;
    a.ent = h->d_ent;
    a.oent = h->d_oent;
    a.sides = h->d_sides;
    a.rowside = h->d_rowside;
    a.N = h->p->d.N;
    // the whole problem
    a.wa = 0;
    a.wb = h->ncn();
    a.pend = a.N;
    a.ostride = a.N;
    a.PH = h->d.PH;
    a.E = h->d.E;
    a.nS = h->nS;
    a.nT = h->nT;
    a.nrows = h->nrows();
    return a;
}

bool needs_fin(const opty_hip_hessmv *h) {
    return h->ntail() > 0 || h->d.nnz_inst > 0 || h->d.T > 0;
}

FinArgs fin_args(const opty_hip_hessmv *h, const double *values,
                 const double *v, double *out) {
    const Pieces s = pieces(h, values);
    FinArgs f{};
    f.part = h->d_part;
    f.ival = s.ival;
    f.pval = s.pval;
    f.v = v;
    f.y = out;
    f.sides = h->d_sides;
    f.irows = h->d_irows;
    f.icols = h->d_icols;
    f.prows = h->d_prows;
    f.pcols = h->d_pcols;
    f.nblk = h->blocks();
    f.tail = (long long)h->nrows()*h->p->d.N;
    // the whole problem: the tail entries end y, and the call owns them
    f.tail_part = out + f.tail;
    f.N = f.pend = f.ostride = h->p->d.N;
    f.wa = 0;
    f.owner = 1;
    f.nS = h->nS;
    f.nT = h->nT;
    f.ntail = h->ntail();
    f.nnz_inst = h->d.nnz_inst;
    f.T = h->d.T;
    return f;
}

// one product on the handle's stream, device pointers
int enqueue_one(opty_hip_hessmv *h, const double *values, const double *v,
                double *out) {
    hipLaunchKernelGGL(opty_hessmv, dim3((unsigned)h->blocks()), dim3(64),
                       h->lds_main, h->stream, main_args(h, values, v, out));
    HIP_TRY(hipGetLastError());
    if (needs_fin(h)) {
        hipLaunchKernelGGL(opty_hessmv_fin, dim3(1), dim3(64), h->lds_fin,
                           h->stream, fin_args(h, values, v, out));
        HIP_TRY(hipGetLastError());
    }
    return 0;
}

// `width` (2 .. Kb) columns in one pass
int enqueue_block(opty_hip_hessmv *h, int width, const double *values,
                  const double *V, long long ldv, double *Y, long long ldy) {
    MvBlockArgs b{main_args(h, values, V, Y), ldv, ldy};
    void *args[] = {&b};
    HIP_TRY(hipLaunchKernel(block_kernel(width), dim3((unsigned)h->blocks()),
                            dim3(64), args,
                            lds_block(h->nS + h->nT, width), h->stream));
    if (needs_fin(h)) {
        FinBlockArgs f{fin_args(h, values, V, Y), ldv, ldy,
                       (long long)h->nT*h->blocks()};
        hipLaunchKernelGGL(opty_hessmv_block_fin, dim3((unsigned)width),
                           dim3(64), h->lds_fin, h->stream, f);
        HIP_TRY(hipGetLastError());
    }
    return 0;
}

}  // namespace

extern "C" {

int opty_hip_hessmv_create(opty_hip_problem *p,
                           const opty_hip_hessmv_desc *desc,
                           opty_hip_hessmv **out) {
    if (!p || !desc || !out) return fail("null argument");
    if (int rc = check_hessmv_desc(p, desc)) return rc;
    const int nrows = p->d.n + p->d.q, ntail = p->d.r + p->d.s;

    // the side table: distinct (row, slot) in ascending order, then the tail
    // offsets in ascending order (hessian_side_table of codegen/program.py)
    std::map<std::pair<int, int>, int> traj, tails;
    auto note = [&](const int32_t *pat, int count, int base) {
        for (int e = 0; e < count; ++e)
            for (int k = 0; k < 2; ++k) {
                const int row = pat[4*e + 2*k], off = pat[4*e + 2*k + 1];
                if (row >= 0) traj[{row, base + off}] = 0;
                else tails[{-1, off}] = 0;
            }
    };
    note(desc->pattern, desc->PH, 0);
    note(desc->obj_pattern, desc->E, desc->obj_base);
    std::vector<int> sides;
    for (auto *m : {&traj, &tails})
        for (auto &kv : *m) {
            kv.second = (int)sides.size()/2;
            sides.push_back(kv.first.first);
            sides.push_back(kv.first.second);
        }
    const int nS = (int)traj.size(), nT = (int)tails.size();
    auto slots = [&](const int32_t *pat, int count, int base) {
        std::vector<int> ent(2*(size_t)count);
        for (int e = 0; e < count; ++e)
            for (int k = 0; k < 2; ++k) {
                const int row = pat[4*e + 2*k], off = pat[4*e + 2*k + 1];
                ent[2*e + k] = row >= 0 ? traj[{row, base + off}]
                                        : tails[{-1, off}];
            }
        return ent;
    };
    const std::vector<int> ent = slots(desc->pattern, desc->PH, 0),
                           oent = slots(desc->obj_pattern, desc->E,
                                        desc->obj_base);
    std::vector<int> rowside(2*(size_t)nrows, -1);
    for (auto &kv : traj) rowside[2*kv.first.first + kv.first.second] =
        kv.second;

    if (int rc = use_device(p)) return rc;
    // LDS: the tile, v and the accumulator per side and lane
    int limit = 0;
    HIP_TRY(hipDeviceGetAttribute(&limit,
                                  hipDeviceAttributeMaxSharedMemoryPerBlock,
                                  p->d.device));
    const size_t lds_main = kTileBytes + (size_t)(nS + nT)*2*64*sizeof(double);
    const size_t lds_fin = (size_t)std::max(1, ntail)*sizeof(double);
    if (lds_main > (size_t)limit)
        return fail("%d sides (%d trajectory, %d tail) need %zu bytes of LDS "
                    "per block, the limit is %d bytes (%d sides)", nS + nT,
                    nS, nT, lds_main, limit,
                    (int)(((size_t)limit - kTileBytes)/(2*64*sizeof(double))));
    if (lds_fin > (size_t)limit)
        return fail("%d tail entries need %zu bytes of LDS, the limit is %d "
                    "bytes", ntail, lds_fin, limit);
    // more than 64 KiB of dynamic LDS has to be asked for
    if (lds_main > 65536)
        HIP_TRY(hipFuncSetAttribute(
            (const void *)opty_hessmv,
            hipFuncAttributeMaxDynamicSharedMemorySize, (int)limit));
    if (lds_fin > 65536)
        HIP_TRY(hipFuncSetAttribute(
            (const void *)opty_hessmv_fin,
            hipFuncAttributeMaxDynamicSharedMemorySize, (int)limit));
    // block products: the widest pass whose LDS fits (hessian_block_width of
    // codegen/program.py), 1: column by column through the kernels above
    int Kb = 1;
    for (int w = kMaxWidth; w >= 2 && Kb == 1; --w)
        if (lds_block(nS + nT, w) <= (size_t)limit) Kb = w;
    for (int w = 2; w <= Kb; ++w)
        if (lds_block(nS + nT, w) > 65536)
            HIP_TRY(hipFuncSetAttribute(
                block_kernel(w), hipFuncAttributeMaxDynamicSharedMemorySize,
                (int)limit));
    if (Kb > 1 && lds_fin > 65536)
        HIP_TRY(hipFuncSetAttribute(
            (const void *)opty_hessmv_block_fin,
            hipFuncAttributeMaxDynamicSharedMemorySize, (int)limit));

    auto *h = new opty_hip_hessmv;
    h->p = p;
    h->device = p->d.device;
    h->d = *desc;
    h->d.pattern = h->d.obj_pattern = nullptr;
    h->d.inst_rows = h->d.inst_cols = h->d.tail_rows = h->d.tail_cols =
        nullptr;
    h->sides = sides;
    h->nS = nS;
    h->nT = nT;
    h->Kb = Kb;
    h->lds_main = lds_main;
    h->lds_fin = lds_fin;
    auto tables = [&]() -> int {
        if (int rc = upload(&h->d_ent, ent.data(), ent.size())) return rc;
        if (int rc = upload(&h->d_oent, oent.data(), oent.size())) return rc;
        if (int rc = upload(&h->d_sides, sides.data(), sides.size()))
            return rc;
        if (int rc = upload(&h->d_rowside, rowside.data(), rowside.size()))
            return rc;
        const size_t ni = (size_t)desc->nnz_inst, nt = (size_t)desc->T;
        if (int rc = upload(&h->d_irows, (const long long *)desc->inst_rows,
                            ni))
            return rc;
        if (int rc = upload(&h->d_icols, (const long long *)desc->inst_cols,
                            ni))
            return rc;
        if (int rc = upload(&h->d_prows, (const long long *)desc->tail_rows,
                            nt))
            return rc;
        if (int rc = upload(&h->d_pcols, (const long long *)desc->tail_cols,
                            nt))
            return rc;
        // one partial per block and tail side, and per column of a pass
        return ensure(&h->d_part, (size_t)nT*(size_t)h->blocks()*(size_t)Kb);
    };
    if (int rc = tables()) {
        (void)opty_hip_hessmv_destroy(h);
        return rc;
    }
    *out = h;
    return 0;
}

int opty_hip_hessmv_destroy(opty_hip_hessmv *h) {
    if (!h) return 0;
    borrowed_destroy(h, {h->d_ent, h->d_oent, h->d_sides, h->d_rowside,
                         h->d_irows, h->d_icols, h->d_prows, h->d_pcols,
                         h->d_part, h->d_val, h->d_v, h->d_y});
    delete h;
    return 0;
}

int64_t opty_hip_hessmv_nnz(const opty_hip_hessmv *h) {
    return h ? h->nnz() : -1;
}

int32_t opty_hip_hessmv_sides(const opty_hip_hessmv *h, int32_t *sides,
                              int32_t room, int32_t *num_trajectory) {
    if (!h) return -1;
    const int32_t count = h->nS + h->nT;
    if (num_trajectory) *num_trajectory = h->nS;
    if (sides)
        for (int32_t k = 0; k < 2*std::min(count, room); ++k)
            sides[k] = h->sides[k];
    return count;
}

int opty_hip_hessmv_apply(opty_hip_hessmv *h, const double *values,
                          const double *v, double *y, int32_t mem) {
    if (!h || !v || !y || (!values && h->nnz() > 0))
        return fail("null argument");
    if (int rc = borrowed_begin(h, mem, false)) return rc;
    const size_t nfree = (size_t)h->p->num_free(), nnz = (size_t)h->nnz();
    double *out = y;
    if (mem == OPTY_HIP_HOST) {
        if (int rc = stage_in(h, &values, &h->d_val, nnz,
                              std::max<size_t>(1, nnz)))
            return rc;
        if (int rc = grow(&h->d_v, &h->cap_v, nfree)) return rc;
        if (int rc = stage_in(h, &v, &h->d_v, nfree, nfree)) return rc;
        if (int rc = grow(&h->d_y, &h->cap_y, nfree)) return rc;
        out = h->d_y;
    }
    if (int rc = enqueue_one(h, values, v, out)) return rc;
    if (mem == OPTY_HIP_HOST) {
        if (int rc = stage_out(h, y, h->d_y, nfree*sizeof(double))) return rc;
        return host_done(h);
    }
    return 0;
}

int opty_hip_hessmv_apply_shard(opty_hip_hessmv *h,
                                const double *values_shard,
                                const double *inst_values, const double *v,
                                double *out, int64_t out_stride,
                                double *tail_part, int64_t node_begin,
                                int64_t node_end, int32_t tail_owner) {
    if (!h || !values_shard || !v || !out) return fail("null argument");
    if (h->d.E != 0 || h->d.T != 0)
        return fail("the handle has an objective section (E %d, T %d): only "
                    "the constraint section is node-sharded", h->d.E, h->d.T);
    if (h->d.nnz_inst > 0 && !inst_values)
        return fail("null inst_values, but the handle has %d instance "
                    "entries", h->d.nnz_inst);
    if (h->ntail() > 0 && !tail_part)
        return fail("null tail_part, but the problem has %d tail entries",
                    h->ntail());
    const int64_t wa = node_begin, wb = node_end;
    if (wa < 0 || wb > (int64_t)h->ncn() || wa > wb)
        return fail("node window [%lld, %lld) is not within the %lld "
                    "constraint nodes", (long long)wa, (long long)wb,
                    h->ncn());
    // the time nodes the window owns: the last window also owns node N - 1
    const int64_t pend = wb > wa ? (int64_t)h->pend(wb) : wb;
    const int64_t owned = pend - wa;
    if (out_stride < owned)
        return fail("out_stride %lld < the %lld time nodes the window owns",
                    (long long)out_stride, (long long)owned);
    const int nrows = h->nrows();
    if (wb > wa && nrows > 0) {
        auto meets = [](const double *a, size_t na, const double *b,
                        size_t nb) {
            const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
            return a0 < b0 + nb*sizeof(double) && b0 < a0 + na*sizeof(double);
        };
        const size_t no = (size_t)(nrows - 1)*(size_t)out_stride +
                          (size_t)owned,
                     nval = (size_t)(wb - wa + (wa > 0 ? 1 : 0))*
                            (size_t)h->d.PH;
        if (meets(out, no, v, (size_t)h->p->num_free()))
            return fail("out (%d rows, out_stride %lld) overlaps v", nrows,
                        (long long)out_stride);
        if (nval && meets(out, no, values_shard, nval))
            return fail("out (%d rows, out_stride %lld) overlaps the %zu "
                        "values of the shard", nrows, (long long)out_stride,
                        nval);
    }
    if (int rc = borrowed_begin(h, OPTY_HIP_DEVICE, false)) return rc;
    const bool fin = h->ntail() > 0 || h->d.nnz_inst > 0;
    FinArgs f = fin_args(h, values_shard, v, out);
    f.ival = inst_values;
    f.pval = nullptr;
    f.tail_part = tail_part;
    f.wa = wa;
    f.pend = pend;
    f.ostride = out_stride;
    f.owner = tail_owner != 0;
    if (wa == wb) {
        // nothing to evaluate: the window's share of the tail sums is zero
        // (all bits clear), on top of which the owner's explicit triplets go
        if (h->ntail() > 0)
            HIP_TRY(hipMemsetAsync(tail_part, 0,
                                   (size_t)h->ntail()*sizeof(double),
                                   h->stream));
        if (!(f.owner && h->d.nnz_inst > 0)) return 0;
        f.nblk = 0;
    } else {
        MvArgs a = main_args(h, values_shard, v, out);
        a.oval = nullptr;
        a.wa = wa;
        a.wb = wb;
        a.pend = pend;
        a.ostride = out_stride;
        f.nblk = h->blocks(wa, wb);
        hipLaunchKernelGGL(opty_hessmv, dim3((unsigned)f.nblk), dim3(64),
                           h->lds_main, h->stream, a);
        HIP_TRY(hipGetLastError());
        if (!fin) return 0;
    }
    hipLaunchKernelGGL(opty_hessmv_fin, dim3(1), dim3(64), h->lds_fin,
                       h->stream, f);
    HIP_TRY(hipGetLastError());
    return 0;
}

int32_t opty_hip_hessmv_block_width(const opty_hip_hessmv *h) {
    return h ? h->Kb : -1;
}

int opty_hip_hessmv_apply_block(opty_hip_hessmv *h, const double *values,
                                const double *V, int64_t ldv,
                                double *Y, int64_t ldy,
                                int32_t ncols, int32_t mem) {
    if (!h || !V || !Y || (!values && h->nnz() > 0))
        return fail("null argument");
    if (ncols < 0) return fail("ncols %d < 0", ncols);
    const int64_t num_free = h->p->num_free();
    if (ldv < num_free)
        return fail("ldv %lld < num_free %lld", (long long)ldv,
                    (long long)num_free);
    if (ldy < num_free)
        return fail("ldy %lld < num_free %lld", (long long)ldy,
                    (long long)num_free);
    const size_t nfree = (size_t)num_free, nnz = (size_t)h->nnz();
    if (ncols > 0) {
        // [first, last) of Y against V and against values
        auto meets = [](const double *a, size_t na, const double *b,
                        size_t nb) {
            const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
            return a0 < b0 + nb*sizeof(double) && b0 < a0 + na*sizeof(double);
        };
        const size_t ny = (size_t)(ncols - 1)*(size_t)ldy + nfree,
                     nv = (size_t)(ncols - 1)*(size_t)ldv + nfree;
        if (meets(Y, ny, V, nv))
            return fail("Y (%d columns, ldy %lld) overlaps V (ldv %lld)",
                        ncols, (long long)ldy, (long long)ldv);
        if (nnz && meets(Y, ny, values, nnz))
            return fail("Y (%d columns, ldy %lld) overlaps the %zu values",
                        ncols, (long long)ldy, nnz);
    }
    if (int rc = borrowed_begin(h, mem, false)) return rc;
    if (ncols == 0) return 0;
    const double *dV = V;
    double *dY = Y;
    long long dldv = ldv, dldy = ldy;
    if (mem == OPTY_HIP_HOST) {
        // the columns without their padding
        if (int rc = stage_in(h, &values, &h->d_val, nnz,
                              std::max<size_t>(1, nnz)))
            return rc;
        if (int rc = grow(&h->d_v, &h->cap_v, (size_t)ncols*nfree)) return rc;
        if (int rc = grow(&h->d_y, &h->cap_y, (size_t)ncols*nfree)) return rc;
        for (int c = 0; c < ncols; ++c)
            HIP_TRY(hipMemcpyAsync(h->d_v + (size_t)c*nfree,
                                   V + (size_t)c*(size_t)ldv,
                                   nfree*sizeof(double),
                                   hipMemcpyHostToDevice, h->stream));
        dV = h->d_v;
        dY = h->d_y;
        dldv = dldy = (long long)nfree;
    }
    // ceil(ncols / Kb) passes; the last one as wide as what is left
    for (int c = 0; c < ncols; c += h->Kb) {
        const int width = std::min(h->Kb, ncols - c);
        const double *vc = dV + (size_t)c*(size_t)dldv;
        double *yc = dY + (size_t)c*(size_t)dldy;
        if (int rc = width == 1 ? enqueue_one(h, values, vc, yc)
                                : enqueue_block(h, width, values, vc, dldv,
                                                yc, dldy))
            return rc;
    }
    if (mem == OPTY_HIP_HOST) {
        for (int c = 0; c < ncols; ++c)
            if (int rc = stage_out(h, Y + (size_t)c*(size_t)ldy,
                                   h->d_y + (size_t)c*nfree,
                                   nfree*sizeof(double)))
                return rc;
        return host_done(h);
    }
    return 0;
}

}  // extern "C"
