// opty_internal.h -- what the translation units of libopty_hip.so share:
// error reporting, the problem handle, the launch / evaluation core's
// prototypes, the base of the handles that borrow a problem handle.  Not
// installed; the public interface is include/opty_hip.h.
//
//   runtime.cpp       handles, kernel launches, routing, the entry points of
//                     the evaluation itself, index kernels, objective and
//                     matrix programs
//   host_scatter.cpp  the host-buffer (cyipopt callback) path: packing on the
//                     device, chunked DMA, the scatter pool of host threads
//                     and its NUMA placement, the segmented layout
//   comm.cpp          RCCL communicator, broadcast of `free`, gather-v
//   hessian.cpp       the Hessian handle (borrows a problem handle)
//   jacprod.cpp       the Jacobian-product handle (J v, J^T w; borrows too)
//   hessmv.cpp        the Hessian-product handle (H v from the stored
//                     triplets; borrows too, kernels of its own)
//   hesscsr.cpp       the CSR-Hessian handle (the triplets compressed to the
//                     unique lower triangle; borrows too, kernels of its own)
//   kktcsr.cpp        the augmented-system handle (CSR Hessian with every
//                     diagonal and CSR Jacobian as one CSR lower triangle;
//                     borrows too, owns a CSR-Hessian handle, kernels of
//                     its own)
//   normal.cpp        the normal-matrix handle (the block-tridiagonal J D^-1
//                     J^T formed, factorised by block cyclic reduction and
//                     solved with; borrows too, kernels of its own)
//   referee.cpp       (libopty_hip_referee.so) instruction-tape kernel and
//                     register poisoner of the build verification
#pragma once
#include <hip/hip_runtime.h>

#include <sched.h>
#include <sys/syscall.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <cctype>
#include <chrono>
#include <condition_variable>
#include <cstdarg>
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <functional>
#include <initializer_list>
#include <mutex>
#include <queue>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#include "../../include/opty_hip.h"

namespace opty {

extern thread_local std::string g_error;
int fail(const char *fmt, ...);

}  // namespace opty

using opty::fail;

#define HIP_TRY(expr)                                                         \
    do {                                                                      \
        hipError_t e_ = (expr);                                               \
        if (e_ != hipSuccess) {                                               \
            (void)hipGetLastError(); /* the runtime's error state is sticky */\
            return fail("%s failed: %s", #expr, hipGetErrorString(e_));       \
        }                                                                     \
    } while (0)

// opty_uni fills the node-invariant table with up to this many single-lane
// workgroups (the generated kernel switches on blockIdx.x; surplus ones exit).
#define OPTY_UNI_WORKGROUPS 16

// The packed kernarg buffer; must match the parameter list every generated
// kernel has (KERNEL_PARAMS in opty_amd/codegen/emit_hip.py).
struct KernelArgs {
    const double *free_;
    const double *known_traj;
    const double *params;
    const double *uni_c;
    double *uni_w;
    const long long *inst_idx;
    double *con;
    double *jac;
    double h;
    long long N;
    long long con_stride;
    long long node_begin;
    long long node_end;
    // kernels with a list schedule only (desc.jac_persist / fused_persist):
    // one more parameter, the schedule table (build_schedule below)
    const int *sched;
};

// one list schedule of a persistent kernel (build_schedule below), on the
// device: per launch size
struct Schedule {
    long long nblk = -1;
    int *d_table = nullptr;
    int npw = 0;
};

// Which kernels the entry points launch for one launch size, measured on
// the device the handle lives on (opty_hip_desc.routing, calibrate_route).
struct Route {
    long long nblk = -1;
    bool var = false;       // the restricted flavour (opty_*_var kernels)
    bool fused_loses = false, jac_via_fused = false;
    float ms_fused = 0.f, ms_con = 0.f, ms_jac = 0.f;   // per launch
};

// A device Jacobian buffer whose owner keeps what the library wrote into it
// (opty_hip_output_register): `valid` = it holds a whole evaluation of the
// node range [begin, end) with the handle's present node-invariant values.
struct RegisteredOutput {
    double *jac = nullptr;
    long long begin = 0, end = 0;
    bool valid = false;
};

struct opty_hip_problem {
    std::vector<Schedule> sched_jac, sched_fused;
    // the restricted kernels in run form (opty_hip_set_restricted_runs): 0 =
    // one workgroup per (block, strip), dispatched by the hardware
    std::vector<Schedule> sched_var_jac, sched_var_fused;
    hipModule_t run_module = nullptr;   // their code object
    int var_jac_persist = 0, var_fused_persist = 0;
    float var_jac_class_cost[OPTY_HIP_MAX_CLASSES] = {},
          var_fused_class_cost[OPTY_HIP_MAX_CLASSES] = {};
    std::vector<Route> routes;
    std::vector<RegisteredOutput> outputs;
    // flavour of the last Jacobian launch per launch size (opty_hip_routing)
    std::vector<std::pair<long long, bool>> served;
    void invalidate_outputs() { for (auto &o : outputs) o.valid = false; }
    hipEvent_t ev_cal0 = nullptr, ev_cal1 = nullptr;
    opty_hip_desc d{};
    hipModule_t module = nullptr;
    hipFunction_t k_con = nullptr, k_jac = nullptr, k_conjac = nullptr,
                  k_inst = nullptr, k_uni = nullptr, k_jac_var = nullptr,
                  k_conjac_var = nullptr;
    hipStream_t own_stream = nullptr, stream = nullptr;
    hipStream_t copy_stream = nullptr;  // device-to-host side of a pipeline
    hipStream_t copy_stream2 = nullptr; // ... its chunks alternate between two
    double *d_params = nullptr, *d_known = nullptr, *d_uni = nullptr;
    bool uni_dirty = true;   // node-invariant table needs (re)computing
    long long *d_inst_idx = nullptr, *d_inst_rows = nullptr,
              *d_inst_cols = nullptr;
    int *d_pattern = nullptr;   // (j, k) per stored block entry when pruned
    // host copies of that pattern and of the instance entries' indices, for
    // the handles that lay the Jacobian out again (kktcsr.cpp)
    std::vector<int32_t> block_jk;
    std::vector<int64_t> inst_rows_host, inst_cols_host;
    int *d_rowinfo = nullptr;   // (S_j, L_j) per stored block entry (CSR)
    double *d_free = nullptr, *d_con = nullptr, *d_jac = nullptr;  // staging
    double *d_con_scratch = nullptr;    // jac_via_fused: discarded values
    long long *d_rows = nullptr, *d_cols = nullptr;                // staging
    double h = 0.0;
    bool have_params = false, have_known = false, have_inst = false,
         have_h = false;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    hipStream_t last_stream = nullptr;   // stream of the last enqueued work
    // host-visible Jacobian by varying entries (opty_hip_eval_jac_persistent)
    std::vector<int> var_entries, run_start, run_len;
    std::vector<int> copy_dst, copy_src;  // opty_hip_set_entry_copies
    std::vector<double> copy_scale;       // ..._scaled (empty: plain copies)
    int *d_var = nullptr;
    double *d_packed = nullptr, *h_packed = nullptr;
    // page-locked, device-mapped staging of the latency path (eval_mapped)
    double *h_free = nullptr, *h_con = nullptr, *h_jac = nullptr;
    // OPTY_HIP_LAYOUT_SEGMENTED (opty_hip_set_segments): block entries in
    // stored order, the lengths of the three segments, for every entry of
    // segment 1 the position in segment 0 it repeats
    std::vector<int> seg_order, seg_copy_src;
    int seg_len[3] = {0, 0, 0};
    bool have_segments = false;
    int *d_seg_order = nullptr;
    double *d_dense = nullptr;   // node-major blocks the kernels write
    double *d_seg = nullptr;     // the same values in segmented order
    std::vector<hipEvent_t> chunk_events;
    std::vector<long long> chunk_bounds;  // node ranges of the DMA chunks
    size_t packed_cap = 0;                // doubles in d_packed / h_packed
    const double *static_host = nullptr;  // vector whose invariant entries
    bool static_valid = false;            // ... are up to date
    const double *shard_host = nullptr;   // the same for a node shard copied
    long long shard_begin = 0, shard_end = 0;   // by opty_hip_shard_jac_to_host
    bool shard_valid = false;

    int64_t ncon_nodes() const { return d.N - 1; }
    int64_t P() const { return (int64_t)d.P; }
    int64_t num_free() const { return (int64_t)(d.n + d.q)*d.N + d.r + d.s; }
    int64_t num_con() const { return (int64_t)d.M*ncon_nodes() + d.num_inst; }
    int64_t nnz() const { return P()*ncon_nodes() + d.nnz_inst; }
};


namespace opty {

struct NodeRange {
    long long begin, end, con_stride;
};

int use_device(const opty_hip_problem *p);
int check_ready(const opty_hip_problem *p);
NodeRange whole(const opty_hip_problem *p);
hipStream_t sync_target(hipStream_t s);
std::vector<int> build_schedule(int persist, long long nblk, int sets,
                                const float *cost);
std::vector<int> build_run_schedule(int persist, long long nblk, int sets,
                                    const float *cost);
int launch_instance(opty_hip_problem *p, const double *free_, double *con_tail,
                    double *jac_tail);
int eval_device(opty_hip_problem *p, int what, const double *free_,
                double *con, double *jac, const NodeRange &rg,
                bool with_inst);
int device_numa_node();
hipError_t pinned_alloc(void **ptr, size_t bytes);
double *mapped_address(double *host);
// host_scatter.cpp
int eval_segmented(opty_hip_problem *p, int what, const double *free_,
                   double *con, double *jac, int mem, bool full);
void scatter_quiesce();

// A handle's device state (node-invariant table, staging buffers) belongs to
// one stream at a time.  When the caller moved the handle to another stream
// (opty_hip_set_stream), work issued there is ordered after everything the
// handle enqueued on the previous one: opty_uni may overwrite the table that
// kernels of the previous stream still read, and the first fill has to be
// visible to the new stream.
template <typename Handle>
int order_streams(Handle *p) {
    if (p->last_stream && p->last_stream != p->stream) {
        // A switch is rare (set-up code, tests): wait for the old stream on
        // the host.  (An event recorded on hipStreamLegacy and waited for
        // on another stream crashed inside the runtime, ROCm 7.0.2; the
        // legacy handle is synchronised through the null stream it stands
        // for.)
        HIP_TRY(hipStreamSynchronize(sync_target(p->last_stream)));
    }
    p->last_stream = p->stream;
    return 0;
}

template <typename T>
int ensure(T **ptr, size_t count) {
    if (*ptr == nullptr && count > 0)
        HIP_TRY(hipMalloc(reinterpret_cast<void **>(ptr), count*sizeof(T)));
    return 0;
}

template <typename T>
int ensure_pinned(T **ptr, size_t count) {
    if (*ptr == nullptr && count > 0)
        HIP_TRY(pinned_alloc(reinterpret_cast<void **>(ptr),
                             count*sizeof(T)));
    return 0;
}

// ---------------------------------------------------------------------------
// Handles that BORROW a problem handle (hessian.cpp, jacprod.cpp): a code
// object of their own, launched on the problem's device data (known
// parameters and trajectories, h, instance atom indices) and on the problem's
// stream, whichever it is at the time of the call.  They embed this base as
// their first base class and add their kernels, descriptor and buffers.
struct Borrowed {
    opty_hip_problem *p = nullptr;
    int device = 0;
    hipModule_t module = nullptr;
    hipStream_t stream = nullptr;
    hipStream_t last_stream = nullptr;   // stream of the last enqueued work
};

struct WantedKernel {
    hipFunction_t *f;
    const char *name;
    bool required;
};

// Loads the code object and looks the kernels up.  `label`: what the message
// of a missing kernel names (null: the kernel itself).  On failure nothing is
// left loaded; the caller deletes its handle.
inline int borrowed_create(Borrowed *b, opty_hip_problem *p, const char *path,
                           std::initializer_list<WantedKernel> wanted,
                           const char *label) {
    b->p = p;
    b->device = p->d.device;
    hipError_t e = hipModuleLoad(&b->module, path);
    if (e != hipSuccess) {
        b->module = nullptr;
        (void)hipGetLastError();
        return fail("hipModuleLoad(%s) failed: %s", path,
                    hipGetErrorString(e));
    }
    for (const WantedKernel &w : wanted)
        if (w.required &&
            hipModuleGetFunction(w.f, b->module, w.name) != hipSuccess) {
            (void)hipGetLastError();    // not left behind for the caller's runtime
            (void)hipModuleUnload(b->module);
            b->module = nullptr;
            return fail("%s missing from %s", label ? label : w.name, path);
        }
    return 0;
}

// Start of every call: the memory kind, the problem's device, (ready: its
// tables are installed,) and the problem's stream, whichever it is now -- the
// staging buffers may still be in use on the one of the previous call.
inline int borrowed_begin(Borrowed *b, int32_t mem, bool ready) {
    if (mem != OPTY_HIP_HOST && mem != OPTY_HIP_DEVICE)
        return fail("bad memory kind %d", mem);
    if (int rc = use_device(b->p)) return rc;
    if (ready)
        if (int rc = check_ready(b->p)) return rc;
    b->stream = b->p->stream;
    return order_streams(b);
}

// Host callers: `count` values of the host vector `*ptr` go to the staging
// vector `*dev` (allocated once, `room` values), which `*ptr` then names.
inline int stage_in(Borrowed *b, const double **ptr, double **dev,
                    size_t count, size_t room) {
    if (int rc = ensure(dev, room)) return rc;
    if (count)
        HIP_TRY(hipMemcpyAsync(*dev, *ptr, count*sizeof(double),
                               hipMemcpyHostToDevice, b->stream));
    *ptr = *dev;
    return 0;
}

// ... and the way back; host_done waits for the copies.
inline int stage_out(Borrowed *b, void *host, const void *dev, size_t bytes) {
    if (bytes)
        HIP_TRY(hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost,
                               b->stream));
    return 0;
}

inline int host_done(Borrowed *b) {
    HIP_TRY(hipStreamSynchronize(sync_target(b->stream)));
    return 0;
}

// The fields every derived kernel's packed arguments share.
template <typename Args>
void borrowed_args(Args *a, const opty_hip_problem *p, const double *dfree) {
    a->free_ = dfree;
    a->known_traj = p->d_known;
    a->params = p->d_params;
    a->inst_idx = p->d_inst_idx;
    a->h = p->h;
    a->N = p->d.N;
}

// Waits for the handle's last work, frees `bufs` and unloads the module
// (touches nothing of the problem handle, which may be gone already).
inline void borrowed_destroy(Borrowed *b, std::initializer_list<void *> bufs) {
    (void)hipSetDevice(b->device);
    if (b->last_stream)
        (void)hipStreamSynchronize(sync_target(b->last_stream));
    for (void *buf : bufs)
        if (buf) (void)hipFree(buf);
    if (b->module) (void)hipModuleUnload(b->module);
}

// ---------------------------------------------------------------------------
// What the handles over the Hessian's triplets share (hessmv.cpp,
// hesscsr.cpp): the checks of an opty_hip_hessmv_desc and the upload of a
// host table.
inline int check_pattern(const char *what, const int32_t *pat, int count,
                         int base, int nrows, int ntail) {
    for (int e = 0; e < count; ++e)
        for (int k = 0; k < 2; ++k) {
            const int row = pat[4*e + 2*k], off = pat[4*e + 2*k + 1];
            if (row < -1 || row >= nrows)
                return fail("%s entry %d: row %d outside [-1, %d)", what, e,
                            row, nrows);
            if (row >= 0 && (base + off < 0 || base + off > 1))
                return fail("%s entry %d: slot %d outside {0, 1}", what, e,
                            base + off);
            if (row < 0 && (off < 0 || off >= ntail))
                return fail("%s entry %d: tail offset %d outside [0, %d)",
                            what, e, off, ntail);
        }
    return 0;
}

inline int check_explicit(const char *what, const int64_t *rows,
                          const int64_t *cols, int count, int64_t num_free) {
    for (int k = 0; k < count; ++k) {
        if (rows[k] < 0 || rows[k] >= num_free || cols[k] < 0 ||
            cols[k] >= num_free)
            return fail("%s entry %d: (%lld, %lld) outside [0, %lld)", what,
                        k, (long long)rows[k], (long long)cols[k],
                        (long long)num_free);
        if (rows[k] < cols[k])
            return fail("%s entry %d: (%lld, %lld) is above the diagonal "
                        "(row < col)", what, k, (long long)rows[k],
                        (long long)cols[k]);
    }
    return 0;
}

// Everything opty_hip_hessmv_create refuses in a descriptor.
inline int check_hessmv_desc(const opty_hip_problem *p,
                             const opty_hip_hessmv_desc *desc) {
    if (desc->PH < 0 || desc->nnz_inst < 0 || desc->E < 0 || desc->T < 0)
        return fail("bad Hessian-product descriptor (PH %d, nnz_inst %d, E "
                    "%d, T %d)", desc->PH, desc->nnz_inst, desc->E, desc->T);
    if (desc->PH > 0 && !desc->pattern) return fail("null index pattern");
    if (desc->E > 0 && !desc->obj_pattern)
        return fail("null objective index pattern");
    if (desc->nnz_inst > 0 && (!desc->inst_rows || !desc->inst_cols))
        return fail("null instance indices");
    if (desc->T > 0 && (!desc->tail_rows || !desc->tail_cols))
        return fail("null parameter-parameter indices");
    if (desc->E > 0 && desc->obj_base != 0 && desc->obj_base != 1)
        return fail("obj_base %d outside {0, 1}", desc->obj_base);
    if (p->d.N < 2) return fail("N %lld < 2", (long long)p->d.N);
    const int nrows = p->d.n + p->d.q, ntail = p->d.r + p->d.s;
    if (int rc = check_pattern("pattern", desc->pattern, desc->PH, 0, nrows,
                               ntail))
        return rc;
    if (int rc = check_pattern("objective pattern", desc->obj_pattern,
                               desc->E, desc->obj_base, nrows, ntail))
        return rc;
    if (int rc = check_explicit("instance", desc->inst_rows, desc->inst_cols,
                                desc->nnz_inst, p->num_free()))
        return rc;
    return check_explicit("parameter-parameter", desc->tail_rows,
                          desc->tail_cols, desc->T, p->num_free());
}

template <typename T>
int upload(T **dev, const T *host, size_t count) {
    if (!count) return 0;
    HIP_TRY(hipMalloc((void **)dev, count*sizeof(T)));
    HIP_TRY(hipMemcpy(*dev, host, count*sizeof(T), hipMemcpyHostToDevice));
    return 0;
}

}  // namespace opty
