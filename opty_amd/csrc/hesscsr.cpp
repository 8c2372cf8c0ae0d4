// hesscsr.cpp -- the CSR-Hessian handle of libopty_hip.so: the stored triplets
// of the Hessian of the Lagrangian compressed to the CSR lower triangle, every
// distinct (row, col) pair once, rows and columns ascending, duplicates summed
// (include/opty_hip.h, "Hessian as CSR").  The value vector is the one of
// hessmv.cpp: [node section | instance entries | objective section |
// parameter-parameter entries].
//
// The handle borrows its problem handle for N, n, q, r, s, device and stream
// and loads no code object: the two kernels below serve every problem.  The
// structure is closed form (hessian_csr_structure of codegen/program.py is the
// host statement).  A SOURCE of an output is a code 2*e + back: entry e of the
// per-node list (node section, then objective section) at node p - back, p
// the time node of the output.
//
//   trajectory row R*N + p, 1 <= p <= N - 2: the entries of row side (R, 0) at
//       node p and those of (R, 1) at node p - 1, merged: L_R columns (R', d),
//       d in {-1, 0, 1}, the same at every such p; the row starts at
//       base_R + (p - 1) L_R + (columns that explicit triplets added before).
//   tail row j: per trajectory row R' it couples with one SEGMENT of
//       consecutive time nodes, column R'*N + p at base + p; then its tail
//       columns.
//   everything else is an ITEM of opty_hesscsr_fin, one output with its list
//       of positions in `values`: the first and the last time node of every
//       trajectory row (a sub-list of the columns), every row that holds an
//       explicit triplet (instance, parameter-parameter), the tail x tail
//       pairs.
//
// opty_hesscsr: lane = time node, one wave per block, blocks of 64 lanes that
// advance by 63 nodes (opty_hessmv's scheme: node p - 1 is in the block; lane
// 0 of a later block repeats a node and stores nothing).  The node entries of
// a row class are one WINDOW of consecutive entries (build_hessian_program
// sorts a node's entries by row side), and consecutive classes share a tile
// while their windows together stay within 64 entries: the window of the
// block's 64 nodes goes through LDS (rows of consecutive doubles in, lane =
// node out, odd pitch), so that every value of a trajectory row is read from
// memory once; the objective section is read straight from memory,
// entry-major.  A wave's outputs of one trajectory row class are runs of L_R
// doubles that follow one another in data: 32 columns at a time go through a
// 64 x 33 tile and leave as one run.  A segment is one coalesced store per
// lane; the few entries of the tail rows are read where they lie.
//
// ORDER OF ADDITION.  A short group (everything but a tail x tail pair with
// per-node sources) adds its triplets in ascending position in `values`,
// starting from +0.0: node p - 1 before node p, ascending entry, then instance
// entries, then the objective section (entry-major), then parameter-parameter
// entries -- the bits of np.add.at(zeros, slot, values).  A long group: per
// node its sources in that order from +0.0; lanes past the last node and the
// repeated lane 0 count as 0.0; per block the tree x[l] += x[l + d], d = 32,
// 16 .. 1 (__shfl_down); opty_hesscsr_fin adds the block partials in block
// order from +0.0, then the explicit triplets in stored order.  Nothing
// depends on anything but N: the same bits in every call and for both memory
// kinds.  Every element of data is stored exactly once, by opty_hesscsr or by
// the item that owns it; no atomics; nothing outside data (and the handle's
// partials) is written.
//
// WITH EVERY DIAGONAL (opty_hip_hesscsr_create_with_diagonal, what kktcsr.cpp
// builds on): an empty source list for (R, 0) in every trajectory row class,
// in every whole row and in every tail row.  (R, 0) is the largest key of a
// class of the lower triangle, so the diagonal is the last column of its row;
// an output without sources is stored as +0.0 by the loops above as they are.
#include "opty_internal.h"

#include <cstdint>
#include <map>
#include <tuple>

using namespace opty;

namespace {

constexpr long long kStride = 63;   // nodes a block advances by
constexpr int kChunk = 32;          // columns of a row class per output tile
constexpr int kPitch = kChunk + 1;  // odd: lane = node writes hit all banks
constexpr int kWindow = 64;         // entries of a node that row classes share

struct CsrArgs {
    const double *val;      // node section, val[i*PH + e]
    const double *oval;     // objective section, oval[e*ncn + j]
    double *data;
    double *part;           // part[b*nL + t]
    const int *srcbeg;      // sources of column c: src[srcbeg[c] .. srcbeg[c+1])
    const int *src;         // 2*e + back
    const int *trcol;       // columns of row class R: trcol[R] .. trcol[R+1]
    const int *trwin;       // (first entry, entries) of the window to load
    const long long *trbase;    // position of row (R, p = 1)
    const int *xbeg;        // interior rows of R that items own: xbeg[R] ..
    const long long *xp;    // ... their time node
    const int *xcnt;        // ... the columns they have beyond L_R
    const long long *segbase;   // output of time node p: segbase[g] + p
    const int *seg;         // (column, first p, 1: last p is N - 1, else N - 2)
    const int *skbeg;       // time nodes of segment g that items own: skbeg[g] ..
    const long long *skp;
    const int *longcol;     // column of long group t
    long long N;
    int PH, pitch, nrows, nseg, nL;
};

// lane = time node; one wave per block
__global__ void __launch_bounds__(64)
opty_hesscsr(CsrArgs a) {
    extern __shared__ double lds[];
    const int lane = threadIdx.x;
    double *tile = lds;                              // [64][pitch], a window
    double *otile = lds + 64*a.pitch;                // [64][kPitch]
    long long *rs = (long long *)(otile + 64*kPitch);   // [64]
    const long long N = a.N, ncn = N - 1;
    const long long i0 = (long long)blockIdx.x*kStride;
    const long long p = i0 + lane;
    // nodes of this block that exist (>= 1: i0 < ncn for every block)
    const int nv = (int)(ncn - i0 < 64 ? ncn - i0 : 64);
    // lane 0 of a later block is lane 63 of the block before
    const bool owner = lane > 0 || blockIdx.x == 0;

    const double *blk = a.val + i0*a.PH;
    int e0 = 0;         // first entry of the window in the tile

    // a source whose node p - back exists: from the tile (lane - back >= 0 for
    // every owner whose node p - back >= 0) or from where it lies
    auto source = [&](int code) {
        const int e = code >> 1, back = code & 1;
        if (e < a.PH) return tile[(lane - back)*a.pitch + e - e0];
        return a.oval[(long long)(e - a.PH)*ncn + p - back];
    };
    auto direct = [&](int code) {
        const int e = code >> 1, back = code & 1;
        if (e < a.PH) return a.val[(p - back)*a.PH + e];
        return a.oval[(long long)(e - a.PH)*ncn + p - back];
    };

    // trajectory rows 1 <= p <= N - 2: both nodes exist
    for (int R = 0; R < a.nrows; ++R) {
        const int c_first = a.trcol[R], L = a.trcol[R + 1] - c_first;
        if (L == 0) continue;
        long long start = -1;
        if (owner && p >= 1 && p < ncn) {
            long long shift = 0;
            bool mine = true;
            for (int x = a.xbeg[R]; x < a.xbeg[R + 1]; ++x) {
                if (a.xp[x] < p) shift += a.xcnt[x];
                else if (a.xp[x] == p) mine = false;
            }
            if (mine) start = a.trbase[R] + (p - 1)*L + shift;
        }
        __syncthreads();        // the stores of the row class before are done
        rs[lane] = start;
        // the window of this and the next row classes (0 entries: the one
        // in the tile serves this class too), the block's nv nodes: element
        // 64 j + lane of the nv x ew window, four loads in flight
        const int ew = a.trwin[2*R + 1];
        if (ew > 0) {
            e0 = a.trwin[2*R];
            const int dn = 64/ew, dc = 64 - dn*ew, count = nv*ew;
            int nd = lane/ew, c = lane - nd*ew;
            for (int at = lane; at < count; at += 4*64) {
                double t[4];
                int to[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    to[u] = -1;
                    if (at + 64*u < count) {
                        to[u] = nd*a.pitch + c;
                        t[u] = blk[(long long)nd*a.PH + e0 + c];
                    }
                    nd += dn;
                    c += dc;
                    if (c >= ew) {
                        c -= ew;
                        ++nd;
                    }
                }
#pragma unroll
                for (int u = 0; u < 4; ++u)
                    if (to[u] >= 0) tile[to[u]] = t[u];
            }
        }
        for (int k0 = 0; k0 < L; k0 += kChunk) {
            const int w = L - k0 < kChunk ? L - k0 : kChunk;
            __syncthreads();
            if (start >= 0)
                for (int k = 0; k < w; ++k) {
                    const int c = c_first + k0 + k;
                    double x = 0.0;
                    for (int s = a.srcbeg[c]; s < a.srcbeg[c + 1]; ++s)
                        x += source(a.src[s]);
                    otile[lane*kPitch + k] = x;
                }
            __syncthreads();
            // element 64 j + lane of the 64 x w tile: rows that follow one
            // another in data leave as one run
            const int dn = 64/w, dc = 64 - dn*w;
            int nd = lane/w, c = lane - nd*w;
            for (int at = lane; at < 64*w; at += 64) {
                const long long r = rs[nd];
                if (r >= 0) a.data[r + k0 + c] = otile[nd*kPitch + c];
                nd += dn;
                c += dc;
                if (c >= w) {
                    c -= w;
                    ++nd;
                }
            }
        }
    }
    __syncthreads();

    // segments of the tail rows: one output per lane
    for (int g = 0; g < a.nseg; ++g) {
        const int c = a.seg[3*g], lo = a.seg[3*g + 1];
        const long long hi = a.seg[3*g + 2] ? ncn : ncn - 1;
        bool mine = owner && p >= lo && p <= hi;
        for (int s = a.skbeg[g]; s < a.skbeg[g + 1]; ++s)
            if (a.skp[s] == p) mine = false;
        if (!mine) continue;
        double x = 0.0;
        for (int s = a.srcbeg[c]; s < a.srcbeg[c + 1]; ++s) {
            const long long i = p - (a.src[s] & 1);
            if (i >= 0 && i < ncn) x += direct(a.src[s]);
        }
        a.data[a.segbase[g] + p] = x;
    }

    // long groups: a fixed tree over the lanes; the repeated node counts once
    for (int t = 0; t < a.nL; ++t) {
        const int c = a.longcol[t];
        double x = 0.0;
        if (owner && p < ncn)
            for (int s = a.srcbeg[c]; s < a.srcbeg[c + 1]; ++s)
                x += direct(a.src[s]);
        for (int d = 32; d >= 1; d >>= 1) x += __shfl_down(x, d);
        if (lane == 0) a.part[(long long)blockIdx.x*a.nL + t] = x;
    }
}

struct FinArgs {
    const double *values;
    const double *part;
    double *data;
    const long long *out;       // position in data of item m
    const int *longof;          // its long group, or -1
    const int *beg;             // its addends: pos[beg[m] .. beg[m+1])
    const long long *pos;       // positions in values, ascending
    long long nblk;
    int nitems, nL;
};

// lane = item, enqueued behind opty_hesscsr: the block partials of the item's
// long group in block order, then its addends in ascending position.
__global__ void __launch_bounds__(64)
opty_hesscsr_fin(FinArgs a) {
    const int m = blockIdx.x*64 + threadIdx.x;
    if (m >= a.nitems) return;
    double x = 0.0;
    const int t = a.longof[m];
    if (t >= 0)
        for (long long b = 0; b < a.nblk; ++b) x += a.part[b*a.nL + t];
    for (int s = a.beg[m]; s < a.beg[m + 1]; ++s) x += a.values[a.pos[s]];
    a.data[a.out[m]] = x;
}

// a side of an entry in the order of its free index (N >= 2): trajectory
// rows first, by row then slot; the tail last (_side_order of program.py)
std::tuple<int, int, int> side_order(int row, int off) {
    return row < 0 ? std::make_tuple(1, off, 0) : std::make_tuple(0, row, off);
}

typedef std::map<long long, std::vector<long long>> Row;   // column -> addends

// one piece of a tail row for the structure: `len` consecutive columns
struct Piece {
    long long col, len;
};

}  // namespace

struct opty_hip_hesscsr : Borrowed {
    opty_hip_hessmv_desc d{};
    int64_t nnz_unique = 0;
    size_t lds_main = 0;
    int pitch = 1, nseg = 0, nL = 0, nitems = 0, ncols = 0;
    // what opty_hip_hesscsr_structure walks: the columns (R', d) of every row
    // class, the rows that items own with their columns, the tail rows
    std::vector<int> trcol;
    std::vector<std::pair<int, int>> colkey;
    std::map<long long, std::vector<long long>> whole;
    std::vector<std::vector<Piece>> tailrow;
    int *d_srcbeg = nullptr, *d_src = nullptr, *d_trcol = nullptr,
        *d_trwin = nullptr, *d_xbeg = nullptr, *d_xcnt = nullptr, *d_seg = nullptr,
        *d_skbeg = nullptr, *d_longcol = nullptr, *d_longof = nullptr,
        *d_beg = nullptr;
    long long *d_trbase = nullptr, *d_xp = nullptr, *d_segbase = nullptr,
              *d_skp = nullptr, *d_out = nullptr, *d_pos = nullptr;
    double *d_part = nullptr;
    double *d_val = nullptr, *d_data = nullptr;     // staging for host callers
    long long ncn() const { return p->d.N - 1; }
    long long blocks() const { return (ncn() + kStride - 1)/kStride; }
    int nrows() const { return p->d.n + p->d.q; }
    int ntail() const { return p->d.r + p->d.s; }
    int64_t nnz() const {
        return (int64_t)(d.PH + d.E)*ncn() + d.nnz_inst + d.T;
    }
};

// Both create entry points.  with_diagonal: every row gets its diagonal pair
// -- an EMPTY source list for (R, 0) in every trajectory row class, in every
// whole row that items own and in every tail row --, so that a pair that no
// triplet hits is stored as +0.0 by the kernels as they are.
static int create_impl(opty_hip_problem *p, const opty_hip_hessmv_desc *desc,
                       bool with_diagonal, opty_hip_hesscsr **out) {
    if (!p || !desc || !out) return fail("null argument");
    if (int rc = check_hessmv_desc(p, desc)) return rc;
    const int nrows = p->d.n + p->d.q, ntail = p->d.r + p->d.s;
    const long long N = p->d.N, ncn = N - 1, tail = (long long)nrows*N;
    const int PH = desc->PH, E = desc->E;
    const double total = (double)(PH + E)*(double)ncn + desc->nnz_inst +
                         desc->T;
    if (total >= 2147483648.0)
        return fail("%.0f triplets: the CSR Hessian takes fewer than 2^31",
                    total);
    const long long inst_at = (long long)PH*ncn,
                    obj_at = inst_at + desc->nnz_inst,
                    par_at = obj_at + (long long)E*ncn;

    // per-node classes: trajectory row R -> {(R', d): sources}, tail row j ->
    // {R': sources} (a segment) and {j': sources} (a long group)
    std::vector<std::map<std::pair<int, int>, std::vector<int>>> traj(nrows);
    std::vector<std::map<int, std::vector<int>>> segs(ntail), longs(ntail);
    for (int e = 0; e < PH + E; ++e) {
        const int32_t *pat = e < PH ? desc->pattern + 4*e
                                    : desc->obj_pattern + 4*(e - PH);
        const int base = e < PH ? 0 : desc->obj_base;
        const int ra = pat[0], oa = pat[1] + (ra >= 0 ? base : 0),
                  rb = pat[2], ob = pat[3] + (rb >= 0 ? base : 0);
        if (side_order(ra, oa) < side_order(rb, ob))
            return fail("%s entry %d: side (%d, %d) against (%d, %d) is "
                        "above the diagonal", e < PH ? "pattern"
                        : "objective pattern", e < PH ? e : e - PH, ra, oa,
                        rb, ob);
        if (ra >= 0) traj[ra][{rb, ob - oa}].push_back(2*e + oa);
        else if (rb >= 0) segs[oa][rb].push_back(2*e + ob);
        else longs[oa][ob].push_back(2*e);
    }
    if (with_diagonal)
        for (int R = 0; R < nrows; ++R) traj[R][{R, 0}];
    // ascending position in `values`: node section, node p - 1 before node
    // p; then the objective section, entry-major
    auto in_order = [&](std::vector<int> codes) {
        auto key = [&](int c) {
            return c >> 1 >= PH ? std::make_tuple(1, c >> 1, 0)
                                : std::make_tuple(0, 1 - (c & 1), c >> 1);
        };
        std::sort(codes.begin(), codes.end(),
                  [&](int x, int y) { return key(x) < key(y); });
        return codes;
    };
    auto position = [&](int code, long long at) {
        const long long e = code >> 1, i = at - (code & 1);
        return e < PH ? i*PH + e : obj_at + (e - PH)*ncn + i;
    };
    auto exists = [&](int code, long long at) {
        const long long i = at - (code & 1);
        return i >= 0 && i < ncn;
    };
    // the regular pattern of trajectory row (R, at)
    auto traj_row = [&](int R, long long at) {
        Row row;
        if (with_diagonal) row[(long long)R*N + at];
        for (const auto &kv : traj[R])
            for (int c : in_order(kv.second))
                if (exists(c, at))
                    row[(long long)kv.first.first*N + at + kv.first.second]
                        .push_back(position(c, at));
        return row;
    };

    // explicit triplets: row -> column -> positions in stored order
    std::map<long long, Row> explicit_;
    for (int k = 0; k < desc->nnz_inst; ++k)
        explicit_[desc->inst_rows[k]][desc->inst_cols[k]].push_back(
            inst_at + k);
    for (int k = 0; k < desc->T; ++k)
        explicit_[desc->tail_rows[k]][desc->tail_cols[k]].push_back(
            par_at + k);

    // whole rows of items: the first and the last time node of every
    // trajectory row, and rows with explicit triplets
    std::map<long long, Row> whole;
    for (int R = 0; R < nrows; ++R)
        for (long long at : {0LL, ncn})
            whole[(long long)R*N + at] = traj_row(R, at);
    for (const auto &kv : explicit_) {
        if (kv.first >= tail) continue;
        if (!whole.count(kv.first))
            whole[kv.first] = traj_row((int)(kv.first/N), kv.first % N);
        for (const auto &cv : kv.second) {
            auto &at = whole[kv.first][cv.first];
            at.insert(at.end(), cv.second.begin(), cv.second.end());
        }
    }

    auto *h = new opty_hip_hesscsr;
    h->p = p;
    h->device = p->d.device;
    h->d = *desc;
    h->d.pattern = h->d.obj_pattern = nullptr;
    h->d.inst_rows = h->d.inst_cols = h->d.tail_rows = h->d.tail_cols =
        nullptr;

    // the tables of both kernels, positions assigned row by row
    std::vector<int> srcbeg{0}, src, trwin, xbeg{0}, xcnt, seg, skbeg{0},
                     longcol, longof, beg{0};
    int widest = 0;     // entries of the widest window
    std::vector<long long> trbase, xp, segbase, skp, iout, ipos;
    auto column = [&](const std::vector<int> &codes) {
        src.insert(src.end(), codes.begin(), codes.end());
        srcbeg.push_back((int)src.size());
        return (int)srcbeg.size() - 2;
    };
    auto item = [&](long long at, std::vector<long long> addends, int t) {
        std::sort(addends.begin(), addends.end());
        iout.push_back(at);
        longof.push_back(t);
        ipos.insert(ipos.end(), addends.begin(), addends.end());
        beg.push_back((int)ipos.size());
    };
    auto items_of = [&](long long row, long long at) {
        std::vector<long long> cols;
        for (const auto &cv : whole[row]) {
            item(at + (long long)cols.size(), cv.second, -1);
            cols.push_back(cv.first);
        }
        h->whole[row] = cols;
        return (long long)cols.size();
    };
    long long cursor = 0;
    h->trcol.push_back(0);
    for (int R = 0; R < nrows; ++R) {
        const long long L = (long long)traj[R].size(), row0 = (long long)R*N;
        int elo = PH, ehi = -1;
        for (const auto &kv : traj[R]) {
            column(in_order(kv.second));
            h->colkey.push_back(kv.first);
            for (int c : kv.second)
                if (c >> 1 < PH) {
                    elo = std::min(elo, c >> 1);
                    ehi = std::max(ehi, c >> 1);
                }
        }
        // (the window of the class alone; grouped below)
        trwin.insert(trwin.end(), {elo, ehi});
        if (ehi >= 0) widest = std::max(widest, ehi - elo + 1);
        h->trcol.push_back((int)h->colkey.size());
        cursor += items_of(row0, cursor);
        trbase.push_back(cursor);
        long long extra = 0;
        for (auto it = whole.upper_bound(row0);
             it != whole.end() && it->first < row0 + ncn; ++it) {
            const long long at = it->first - row0;
            const long long len = items_of(it->first,
                                           cursor + (at - 1)*L + extra);
            xp.push_back(at);
            xcnt.push_back((int)(len - L));
            extra += len - L;
        }
        xbeg.push_back((int)xp.size());
        cursor += (ncn - 1)*L + extra;
        cursor += items_of(row0 + ncn, cursor);
    }
    h->tailrow.resize(ntail);
    for (int j = 0; j < ntail; ++j) {
        // segments and explicit columns outside them, in column order
        struct Seg {
            int Rp, lo;
            long long hi;
            std::vector<int> codes;
            Row on;
        };
        std::map<long long, Seg> pieces;    // first column -> segment
        Row extra, tcols;
        for (const auto &kv : segs[j]) {
            Seg s{kv.first, 1, ncn - 1, in_order(kv.second), {}};
            for (int c : s.codes) {
                if (c & 1) s.hi = ncn;
                else s.lo = 0;
            }
            pieces[(long long)s.Rp*N + s.lo] = s;
        }
        for (const auto &kv : longs[j]) tcols[kv.first];
        if (with_diagonal) tcols[j];
        auto found = explicit_.find(tail + j);
        if (found != explicit_.end())
            for (const auto &cv : found->second) {
                if (cv.first >= tail) {
                    auto &at = tcols[cv.first - tail];
                    at.insert(at.end(), cv.second.begin(), cv.second.end());
                    continue;
                }
                Seg *hit = nullptr;
                for (auto &sv : pieces)
                    if (sv.second.Rp == cv.first/N &&
                        sv.second.lo <= cv.first % N &&
                        cv.first % N <= sv.second.hi)
                        hit = &sv.second;
                if (hit) hit->on[cv.first % N] = cv.second;
                else extra[cv.first] = cv.second;
            }
        auto ex = extra.begin();
        auto extras_below = [&](long long colmax) {
            for (; ex != extra.end() && ex->first < colmax; ++ex) {
                item(cursor++, ex->second, -1);
                h->tailrow[j].push_back({ex->first, 1});
            }
        };
        for (auto &sv : pieces) {
            Seg &s = sv.second;
            extras_below(sv.first);
            const int c = column(s.codes);
            segbase.push_back(cursor - s.lo);
            seg.insert(seg.end(), {c, s.lo, s.hi == ncn ? 1 : 0});
            for (const auto &ov : s.on) {
                std::vector<long long> addends = ov.second;
                for (int code : s.codes)
                    if (exists(code, ov.first))
                        addends.push_back(position(code, ov.first));
                item(cursor - s.lo + ov.first, addends, -1);
                skp.push_back(ov.first);
            }
            skbeg.push_back((int)skp.size());
            h->tailrow[j].push_back({sv.first, s.hi - s.lo + 1});
            cursor += s.hi - s.lo + 1;
        }
        extras_below(tail);
        for (const auto &tv : tcols) {
            int t = -1;
            auto lg = longs[j].find((int)tv.first);
            if (lg != longs[j].end()) {
                t = (int)longcol.size();
                longcol.push_back(column(in_order(lg->second)));
            }
            item(cursor++, tv.second, t);
            h->tailrow[j].push_back({tail + tv.first, 1});
        }
    }
    h->nnz_unique = cursor;
    // consecutive row classes share a tile while their windows together stay
    // within kWindow entries (or the widest class's): the first class of a
    // group with columns loads (first entry, entries), the others (-, 0)
    {
        const int room = std::max(widest, kWindow);
        int first = -1, lo = 0, hi = -1;
        auto close = [&]() {
            if (first >= 0) {
                trwin[2*first] = lo;
                trwin[2*first + 1] = hi - lo + 1;
                widest = std::max(widest, hi - lo + 1);
            }
            first = -1;
        };
        for (int R = 0; R < nrows; ++R) {
            const int elo = trwin[2*R], ehi = trwin[2*R + 1];
            trwin[2*R] = trwin[2*R + 1] = 0;
            if (traj[R].empty() || ehi < 0) continue;   // nothing to read
            if (first >= 0 &&
                std::max(hi, ehi) - std::min(lo, elo) + 1 > room)
                close();
            if (first < 0) {
                first = R;
                lo = elo;
                hi = ehi;
            } else {
                lo = std::min(lo, elo);
                hi = std::max(hi, ehi);
            }
        }
        close();
    }
    h->pitch = widest | 1;
    h->nseg = (int)segbase.size();
    h->nL = (int)longcol.size();
    h->nitems = (int)iout.size();
    h->ncols = (int)srcbeg.size() - 1;
    h->lds_main = (size_t)(64*h->pitch + 64*kPitch + 64)*sizeof(double);

    // what the kernels index with stays inside data and values
    auto inside = [&]() -> int {
        for (int R = 0; R < nrows; ++R) {
            const long long L = h->trcol[R + 1] - h->trcol[R];
            long long extra = 0;
            for (int x = xbeg[R]; x < xbeg[R + 1]; ++x) extra += xcnt[x];
            if (trbase[R] < 0 || trbase[R] + (ncn - 1)*L + extra > cursor)
                return fail("row class %d leaves the %lld values of data", R,
                            cursor);
        }
        for (size_t g = 0; g < segbase.size(); ++g)
            if (segbase[g] + seg[3*g + 1] < 0 ||
                segbase[g] + (seg[3*g + 2] ? ncn : ncn - 1) >= cursor)
                return fail("segment %zu leaves the %lld values of data", g,
                            cursor);
        for (long long at : iout)
            if (at < 0 || at >= cursor)
                return fail("an item at %lld leaves the %lld values of data",
                            at, cursor);
        for (long long at : ipos)
            if (at < 0 || at >= (long long)total)
                return fail("an addend at %lld leaves the %.0f values", at,
                            total);
        return 0;
    };
    auto device_side = [&]() -> int {
        if (int rc = inside()) return rc;
        if (int rc = use_device(p)) return rc;
        int limit = 0;
        HIP_TRY(hipDeviceGetAttribute(
            &limit, hipDeviceAttributeMaxSharedMemoryPerBlock, p->d.device));
        if (h->lds_main > (size_t)limit)
            return fail("a row class whose node entries span %d consecutive "
                        "entries needs %zu bytes of LDS per block, the limit "
                        "is %d bytes (%d entries)", widest, h->lds_main, limit,
                        (int)(((size_t)limit/sizeof(double) - 64*kPitch - 64)
                              /64 - 1));
        // more than 64 KiB of dynamic LDS has to be asked for
        if (h->lds_main > 65536)
            HIP_TRY(hipFuncSetAttribute(
                (const void *)opty_hesscsr,
                hipFuncAttributeMaxDynamicSharedMemorySize, (int)limit));
        if (int rc = upload(&h->d_srcbeg, srcbeg.data(), srcbeg.size()))
            return rc;
        if (int rc = upload(&h->d_src, src.data(), src.size())) return rc;
        if (int rc = upload(&h->d_trcol, h->trcol.data(), h->trcol.size()))
            return rc;
        if (int rc = upload(&h->d_trwin, trwin.data(), trwin.size()))
            return rc;
        if (int rc = upload(&h->d_trbase, trbase.data(), trbase.size()))
            return rc;
        if (int rc = upload(&h->d_xbeg, xbeg.data(), xbeg.size())) return rc;
        if (int rc = upload(&h->d_xp, xp.data(), xp.size())) return rc;
        if (int rc = upload(&h->d_xcnt, xcnt.data(), xcnt.size())) return rc;
        if (int rc = upload(&h->d_segbase, segbase.data(), segbase.size()))
            return rc;
        if (int rc = upload(&h->d_seg, seg.data(), seg.size())) return rc;
        if (int rc = upload(&h->d_skbeg, skbeg.data(), skbeg.size()))
            return rc;
        if (int rc = upload(&h->d_skp, skp.data(), skp.size())) return rc;
        if (int rc = upload(&h->d_longcol, longcol.data(), longcol.size()))
            return rc;
        if (int rc = upload(&h->d_out, iout.data(), iout.size())) return rc;
        if (int rc = upload(&h->d_longof, longof.data(), longof.size()))
            return rc;
        if (int rc = upload(&h->d_beg, beg.data(), beg.size())) return rc;
        if (int rc = upload(&h->d_pos, ipos.data(), ipos.size())) return rc;
        // one partial per block and long group
        return ensure(&h->d_part, (size_t)h->nL*(size_t)h->blocks());
    };
    if (int rc = device_side()) {
        (void)opty_hip_hesscsr_destroy(h);
        return rc;
    }
    *out = h;
    return 0;
}

extern "C" {

int opty_hip_hesscsr_create(opty_hip_problem *p,
                            const opty_hip_hessmv_desc *desc,
                            opty_hip_hesscsr **out) {
    return create_impl(p, desc, false, out);
}

int opty_hip_hesscsr_create_with_diagonal(opty_hip_problem *p,
                                          const opty_hip_hessmv_desc *desc,
                                          opty_hip_hesscsr **out) {
    return create_impl(p, desc, true, out);
}

int opty_hip_hesscsr_destroy(opty_hip_hesscsr *h) {
    if (!h) return 0;
    borrowed_destroy(h, {h->d_srcbeg, h->d_src, h->d_trcol, h->d_trwin,
                         h->d_trbase,
                         h->d_xbeg, h->d_xp, h->d_xcnt, h->d_segbase,
                         h->d_seg, h->d_skbeg, h->d_skp, h->d_longcol,
                         h->d_out, h->d_longof, h->d_beg, h->d_pos,
                         h->d_part, h->d_val, h->d_data});
    delete h;
    return 0;
}

int64_t opty_hip_hesscsr_nnz(const opty_hip_hesscsr *h) {
    return h ? h->nnz() : -1;
}

int64_t opty_hip_hesscsr_nnz_unique(const opty_hip_hesscsr *h) {
    return h ? h->nnz_unique : -1;
}

int opty_hip_hesscsr_structure(opty_hip_hesscsr *h, int64_t *indptr,
                               int64_t *indices, int32_t mem) {
    if (!h || !indptr || (!indices && h->nnz_unique > 0))
        return fail("null argument");
    if (int rc = borrowed_begin(h, mem, false)) return rc;
    const long long N = h->p->d.N;
    const size_t nfree = (size_t)h->p->num_free();
    std::vector<int64_t> ptr(nfree + 1), idx((size_t)h->nnz_unique);
    size_t at = 0;
    for (int R = 0; R < h->nrows(); ++R)
        for (long long t = 0; t < N; ++t) {
            const long long row = (long long)R*N + t;
            ptr[(size_t)row] = (int64_t)at;
            auto it = h->whole.find(row);
            if (it != h->whole.end())
                for (long long c : it->second) idx[at++] = c;
            else
                for (int c = h->trcol[R]; c < h->trcol[R + 1]; ++c)
                    idx[at++] = (long long)h->colkey[c].first*N + t +
                                h->colkey[c].second;
        }
    for (int j = 0; j < h->ntail(); ++j) {
        ptr[(size_t)h->nrows()*(size_t)N + j] = (int64_t)at;
        for (const Piece &pc : h->tailrow[j])
            for (long long t = 0; t < pc.len; ++t) idx[at++] = pc.col + t;
    }
    ptr[nfree] = (int64_t)at;
    if (at != (size_t)h->nnz_unique)
        return fail("the CSR structure has %zu columns, the handle counted "
                    "%lld", at, (long long)h->nnz_unique);
    if (mem == OPTY_HIP_HOST) {
        std::memcpy(indptr, ptr.data(), ptr.size()*sizeof(int64_t));
        if (!idx.empty())
            std::memcpy(indices, idx.data(), idx.size()*sizeof(int64_t));
        return 0;
    }
    // (the vectors end with this call: the copies are waited for)
    HIP_TRY(hipMemcpyAsync(indptr, ptr.data(), ptr.size()*sizeof(int64_t),
                           hipMemcpyHostToDevice, h->stream));
    if (!idx.empty())
        HIP_TRY(hipMemcpyAsync(indices, idx.data(),
                               idx.size()*sizeof(int64_t),
                               hipMemcpyHostToDevice, h->stream));
    return host_done(h);
}

int opty_hip_hesscsr_compress(opty_hip_hesscsr *h, const double *values,
                              double *data, int32_t mem) {
    if (!h || !values || !data) return fail("null argument");
    const size_t nnz = (size_t)h->nnz(), nu = (size_t)h->nnz_unique;
    const uintptr_t v0 = (uintptr_t)values, d0 = (uintptr_t)data;
    if (v0 < d0 + nu*sizeof(double) && d0 < v0 + nnz*sizeof(double))
        return fail("data (%zu values) overlaps the %zu values", nu, nnz);
    if (int rc = borrowed_begin(h, mem, false)) return rc;
    double *out = data;
    if (mem == OPTY_HIP_HOST) {
        if (int rc = stage_in(h, &values, &h->d_val, nnz,
                              std::max<size_t>(1, nnz)))
            return rc;
        if (int rc = ensure(&h->d_data, std::max<size_t>(1, nu))) return rc;
        out = h->d_data;
    }
    if (h->ncols > 0) {
        CsrArgs a{};
        a.val = values;
        a.oval = values + (size_t)h->d.PH*h->ncn() + h->d.nnz_inst;
        a.data = out;
        a.part = h->d_part;
        a.srcbeg = h->d_srcbeg;
        a.src = h->d_src;
        a.trcol = h->d_trcol;
        a.trwin = h->d_trwin;
        a.trbase = h->d_trbase;
        a.xbeg = h->d_xbeg;
        a.xp = h->d_xp;
        a.xcnt = h->d_xcnt;
        a.segbase = h->d_segbase;
        a.seg = h->d_seg;
        a.skbeg = h->d_skbeg;
        a.skp = h->d_skp;
        a.longcol = h->d_longcol;
        a.N = h->p->d.N;
        a.PH = h->d.PH;
        a.pitch = h->pitch;
        a.nrows = h->nrows();
        a.nseg = h->nseg;
        a.nL = h->nL;
        hipLaunchKernelGGL(opty_hesscsr, dim3((unsigned)h->blocks()),
                           dim3(64), h->lds_main, h->stream, a);
        HIP_TRY(hipGetLastError());
    }
    if (h->nitems > 0) {
        FinArgs f{};
        f.values = values;
        f.part = h->d_part;
        f.data = out;
        f.out = h->d_out;
        f.longof = h->d_longof;
        f.beg = h->d_beg;
        f.pos = h->d_pos;
        f.nblk = h->blocks();
        f.nitems = h->nitems;
        f.nL = h->nL;
        hipLaunchKernelGGL(opty_hesscsr_fin,
                           dim3((unsigned)((h->nitems + 63)/64)), dim3(64),
                           0, h->stream, f);
        HIP_TRY(hipGetLastError());
    }
    if (mem == OPTY_HIP_HOST) {
        if (int rc = stage_out(h, data, h->d_data, nu*sizeof(double)))
            return rc;
        return host_done(h);
    }
    return 0;
}

}  // extern "C"
