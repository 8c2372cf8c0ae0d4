// programs.cpp -- the other generated programs libopty_hip.so drives:
// the objective / objective gradient (SURVEY.md 8(f) rank 1,
// opty/utils.py:329-470), the objective's exact Hessian and plain matrix
// functions in the reference's
// ufuncify_matrix call shape (opty/utils.py:639-640).
#include "opty_internal.h"

using namespace opty;

// ---------------------------------------------------------------------------
// objective / objective gradient
// ---------------------------------------------------------------------------
struct opty_hip_objective {
    opty_hip_objective_desc d{};
    hipModule_t module = nullptr;
    hipFunction_t k_grad = nullptr, k_fin = nullptr;
    hipStream_t own_stream = nullptr, stream = nullptr;
    hipStream_t last_stream = nullptr;   // stream of the last enqueued work
    double *d_partial = nullptr, *d_value = nullptr;
    double *d_free = nullptr, *d_grad = nullptr;   // staging for host callers
    long long nblk = 0;
    int64_t num_free() const { return (int64_t)(d.n + d.q)*d.N + d.r; }
};

extern "C" {

int opty_hip_objective_create(const opty_hip_objective_desc *desc,
                              const char *code_object_path,
                              opty_hip_objective **out) {
    if (!desc || !code_object_path || !out) return fail("null argument");
    if (desc->N < 2) return fail("need at least 2 collocation nodes");
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count == 0)
        return fail("no HIP device is visible: the HIP backend has no CPU "
                    "fallback");
    if (desc->device < 0 || desc->device >= count)
        return fail("device %d out of range (have %d)", desc->device, count);
    HIP_TRY(hipSetDevice(desc->device));
    auto *o = new opty_hip_objective;
    o->d = *desc;
    hipError_t e = hipModuleLoad(&o->module, code_object_path);
    if (e != hipSuccess) {
        delete o;
        (void)hipGetLastError();
        return fail("hipModuleLoad(%s) failed: %s", code_object_path,
                    hipGetErrorString(e));
    }
    if (hipModuleGetFunction(&o->k_grad, o->module, "opty_objgrad") !=
            hipSuccess ||
        hipModuleGetFunction(&o->k_fin, o->module, "opty_objfin") !=
            hipSuccess) {
        (void)hipModuleUnload(o->module);
        delete o;
        return fail("opty_objgrad/opty_objfin missing from %s",
                    code_object_path);
    }
    auto allocate = [&]() -> int {
        HIP_TRY(hipStreamCreateWithFlags(&o->own_stream,
                                         hipStreamNonBlocking));
        o->stream = o->own_stream;
        o->nblk = (desc->N + 63)/64;
        HIP_TRY(hipMalloc((void **)&o->d_partial,
                          (size_t)o->nblk*(1 + desc->r)*sizeof(double)));
        HIP_TRY(hipMalloc((void **)&o->d_value, sizeof(double)));
        return 0;
    };
    if (int rc = allocate()) {
        (void)opty_hip_objective_destroy(o);
        return rc;
    }
    *out = o;
    return 0;
}

int opty_hip_objective_destroy(opty_hip_objective *o) {
    if (!o) return 0;
    (void)hipSetDevice(o->d.device);
    (void)hipStreamSynchronize(sync_target(o->stream));
    void *bufs[] = {o->d_partial, o->d_value, o->d_free, o->d_grad};
    for (void *b : bufs)
        if (b) (void)hipFree(b);
    if (o->own_stream) (void)hipStreamDestroy(o->own_stream);
    if (o->module) (void)hipModuleUnload(o->module);
    delete o;
    return 0;
}

int opty_hip_objective_set_stream(opty_hip_objective *o, void *hip_stream) {
    if (!o) return fail("null handle");
    o->stream = hip_stream ? (hipStream_t)hip_stream : o->own_stream;
    return 0;
}

int opty_hip_objective_eval(opty_hip_objective *o, const double *free_,
                            double *value, double *grad, int32_t mem) {
    if (!o || !free_ || !value) return fail("null argument");
    HIP_TRY(hipSetDevice(o->d.device));
    // d_partial / d_value (and the staging buffers) may still be in use on
    // the stream the handle was on before opty_hip_objective_set_stream
    if (int rc = order_streams(o)) return rc;
    const double *dfree = free_;
    double *dgrad = grad;
    if (mem == OPTY_HIP_HOST) {
        if (int rc = ensure(&o->d_free, (size_t)o->num_free())) return rc;
        HIP_TRY(hipMemcpyAsync(o->d_free, free_, o->num_free()*sizeof(double),
                               hipMemcpyHostToDevice, o->stream));
        dfree = o->d_free;
        if (grad) {
            if (int rc = ensure(&o->d_grad, (size_t)o->num_free())) return rc;
            dgrad = o->d_grad;
        }
    } else if (mem != OPTY_HIP_DEVICE) {
        return fail("bad memory kind %d", mem);
    }
    KernelArgs a{};
    a.free_ = dfree;
    a.uni_w = o->d_value;
    a.con = o->d_partial;
    a.jac = dgrad;
    a.h = o->d.h;
    a.N = o->d.N;
    a.con_stride = o->nblk;
    a.node_begin = 0;
    a.node_end = o->d.N;
    size_t size = sizeof a;
    void *config[] = {HIP_LAUNCH_PARAM_BUFFER_POINTER, &a,
                      HIP_LAUNCH_PARAM_BUFFER_SIZE, &size,
                      HIP_LAUNCH_PARAM_END};
    HIP_TRY(hipModuleLaunchKernel(o->k_grad, (unsigned)o->nblk, 1, 1, 64, 1, 1,
                                  0, o->stream, nullptr, config));
    HIP_TRY(hipModuleLaunchKernel(o->k_fin, 1, 1, 1, 64, 1, 1, 0, o->stream,
                                  nullptr, config));
    HIP_TRY(hipMemcpyAsync(value, o->d_value, sizeof(double),
                           hipMemcpyDeviceToHost, o->stream));
    if (mem == OPTY_HIP_HOST && grad)
        HIP_TRY(hipMemcpyAsync(grad, o->d_grad, o->num_free()*sizeof(double),
                               hipMemcpyDeviceToHost, o->stream));
    HIP_TRY(hipStreamSynchronize(sync_target(o->stream)));
    return 0;
}

}  // extern "C"

// ---------------------------------------------------------------------------
// exact Hessian of the objective (lower triangle, triplets)
// ---------------------------------------------------------------------------
namespace {

// The packed kernarg buffer of opty_objhess / opty_objhess_fin; must match
// OBJHESS_PARAMS in opty_amd/objective.py.
struct ObjHessArgs {
    const double *free_;
    double *partial;
    double *out;
    double h;
    double factor;
    long long N;
    long long nblk;
};
static_assert(sizeof(ObjHessArgs) == 56, "ObjHessArgs must match "
                                         "OBJHESS_PARAMS");

// Closed-form indices: per-point entry e at quadrature point j (value
// e*npts + j) has the global indices side(pattern[4e], pattern[4e+1]) and
// side(pattern[4e+2], pattern[4e+3]), side(var, off) = var*N + j + base + off,
// or tail + off for var == -1; the T parameter pairs follow.  grid.y = entry
// (the last row: the pairs): consecutive lanes write consecutive int64s.
__global__ void __launch_bounds__(256)
opty_objhess_indices_kernel(const int *pattern, int E, int T, long long N,
                            long long npts, int base, long long tail,
                            long long *rows, long long *cols) {
    const long long j = (long long)blockIdx.x*blockDim.x + threadIdx.x;
    const int e = blockIdx.y;
    if (e < E) {
        if (j >= npts) return;
        const int ra = pattern[4*e], oa = pattern[4*e + 1];
        const int rb = pattern[4*e + 2], ob = pattern[4*e + 3];
        rows[e*npts + j] = ra >= 0 ? (long long)ra*N + j + base + oa
                                   : tail + oa;
        cols[e*npts + j] = rb >= 0 ? (long long)rb*N + j + base + ob
                                   : tail + ob;
    } else if (j < T) {
        rows[E*npts + j] = tail + pattern[4*E + 2*j];
        cols[E*npts + j] = tail + pattern[4*E + 2*j + 1];
    }
}

}  // namespace

struct opty_hip_objhess {
    opty_hip_objhess_desc d{};
    hipModule_t module = nullptr;
    hipFunction_t k_hess = nullptr, k_fin = nullptr;
    hipStream_t own_stream = nullptr, stream = nullptr;
    hipStream_t last_stream = nullptr;   // stream of the last enqueued work
    int *d_pattern = nullptr;            // 4 E + 2 T int32
    double *d_partial = nullptr;
    // staging for host callers
    double *d_free = nullptr, *d_out = nullptr;
    long long *d_rows = nullptr, *d_cols = nullptr;
    long long nblk = 0;
    int64_t npts() const { return d.N - 1; }
    int64_t num_free() const { return (int64_t)(d.n + d.q)*d.N + d.r; }
    int64_t nnz() const { return (int64_t)d.E*npts() + d.T; }
};

extern "C" {

int opty_hip_objhess_create(const opty_hip_objhess_desc *desc,
                            const int32_t *pattern,
                            const char *code_object_path,
                            opty_hip_objhess **out) {
    if (!desc || !code_object_path || !out) return fail("null argument");
    if (desc->N < 2) return fail("need at least 2 collocation nodes");
    if (desc->n < 0 || desc->q < 0 || desc->r < 0 || desc->E < 0 ||
        desc->T < 0 || (desc->base != 0 && desc->base != 1))
        return fail("bad objective Hessian descriptor (n %d, q %d, r %d, "
                    "base %d, E %d, T %d)", desc->n, desc->q, desc->r,
                    desc->base, desc->E, desc->T);
    if ((desc->E > 0 || desc->T > 0) && !pattern)
        return fail("null index pattern");
    // every index has to be a free index at every quadrature point
    for (int e = 0; e < desc->E; ++e)
        for (int s = 0; s < 2; ++s) {
            const int var = pattern[4*e + 2*s], off = pattern[4*e + 2*s + 1];
            const bool ok = var == -1 ? (off >= 0 && off < desc->r)
                : (var >= 0 && var < desc->n + desc->q && off >= 0 &&
                   off + desc->base <= 1);
            if (!ok)
                return fail("index pattern entry %d (%d, %d) is outside the "
                            "free vector", e, var, off);
        }
    for (int t = 0; t < 2*desc->T; ++t)
        if (pattern[4*desc->E + t] < 0 || pattern[4*desc->E + t] >= desc->r)
            return fail("parameter pair %d names parameter %d of %d", t/2,
                        pattern[4*desc->E + t], desc->r);
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count == 0)
        return fail("no HIP device is visible: the HIP backend has no CPU "
                    "fallback");
    if (desc->device < 0 || desc->device >= count)
        return fail("device %d out of range (have %d)", desc->device, count);
    HIP_TRY(hipSetDevice(desc->device));
    auto *o = new opty_hip_objhess;
    o->d = *desc;
    hipError_t e = hipModuleLoad(&o->module, code_object_path);
    if (e != hipSuccess) {
        delete o;
        (void)hipGetLastError();
        return fail("hipModuleLoad(%s) failed: %s", code_object_path,
                    hipGetErrorString(e));
    }
    if (hipModuleGetFunction(&o->k_hess, o->module, "opty_objhess") !=
            hipSuccess ||
        (desc->T > 0 &&
         hipModuleGetFunction(&o->k_fin, o->module, "opty_objhess_fin") !=
             hipSuccess)) {
        (void)hipGetLastError();
        (void)hipModuleUnload(o->module);
        delete o;
        return fail("opty_objhess/opty_objhess_fin missing from %s",
                    code_object_path);
    }
    auto allocate = [&]() -> int {
        HIP_TRY(hipStreamCreateWithFlags(&o->own_stream,
                                         hipStreamNonBlocking));
        o->stream = o->own_stream;
        o->nblk = (desc->N - 1 + 63)/64;
        const size_t words = (size_t)4*desc->E + (size_t)2*desc->T;
        if (words > 0) {
            HIP_TRY(hipMalloc((void **)&o->d_pattern, words*sizeof(int)));
            HIP_TRY(hipMemcpy(o->d_pattern, pattern, words*sizeof(int),
                              hipMemcpyHostToDevice));
        }
        if (desc->T > 0)
            HIP_TRY(hipMalloc((void **)&o->d_partial,
                              (size_t)o->nblk*desc->T*sizeof(double)));
        return 0;
    };
    if (int rc = allocate()) {
        (void)opty_hip_objhess_destroy(o);
        return rc;
    }
    *out = o;
    return 0;
}

int opty_hip_objhess_destroy(opty_hip_objhess *o) {
    if (!o) return 0;
    (void)hipSetDevice(o->d.device);
    if (o->last_stream)
        (void)hipStreamSynchronize(sync_target(o->last_stream));
    void *bufs[] = {o->d_pattern, o->d_partial, o->d_free, o->d_out,
                    o->d_rows, o->d_cols};
    for (void *b : bufs)
        if (b) (void)hipFree(b);
    if (o->own_stream) (void)hipStreamDestroy(o->own_stream);
    if (o->module) (void)hipModuleUnload(o->module);
    delete o;
    return 0;
}

int opty_hip_objhess_set_stream(opty_hip_objhess *o, void *hip_stream) {
    if (!o) return fail("null handle");
    o->stream = hip_stream ? (hipStream_t)hip_stream : o->own_stream;
    return 0;
}

int64_t opty_hip_objhess_nnz(const opty_hip_objhess *o) {
    return o ? o->nnz() : -1;
}

int opty_hip_objhess_indices(opty_hip_objhess *o, int64_t *rows,
                             int64_t *cols, int32_t mem) {
    if (!o || !rows || !cols) return fail("null argument");
    if (mem != OPTY_HIP_HOST && mem != OPTY_HIP_DEVICE)
        return fail("bad memory kind %d", mem);
    HIP_TRY(hipSetDevice(o->d.device));
    if (int rc = order_streams(o)) return rc;
    const size_t nnz = (size_t)o->nnz();
    if (nnz == 0) return 0;
    long long *dr = (long long *)rows, *dc = (long long *)cols;
    if (mem == OPTY_HIP_HOST) {
        if (int rc = ensure(&o->d_rows, nnz)) return rc;
        if (int rc = ensure(&o->d_cols, nnz)) return rc;
        dr = o->d_rows;
        dc = o->d_cols;
    }
    const long long npts = o->npts();
    const long long span = std::max<long long>(npts, o->d.T);
    hipLaunchKernelGGL(opty_objhess_indices_kernel,
                       dim3((unsigned)((span + 255)/256),
                            (unsigned)(o->d.E + (o->d.T > 0 ? 1 : 0))),
                       dim3(256), 0, o->stream, o->d_pattern, o->d.E, o->d.T,
                       (long long)o->d.N, npts, o->d.base,
                       (long long)(o->d.n + o->d.q)*o->d.N, dr, dc);
    HIP_TRY(hipGetLastError());
    if (mem == OPTY_HIP_HOST) {
        HIP_TRY(hipMemcpyAsync(rows, dr, nnz*sizeof(long long),
                               hipMemcpyDeviceToHost, o->stream));
        HIP_TRY(hipMemcpyAsync(cols, dc, nnz*sizeof(long long),
                               hipMemcpyDeviceToHost, o->stream));
        HIP_TRY(hipStreamSynchronize(sync_target(o->stream)));
    }
    return 0;
}

int opty_hip_objhess_eval(opty_hip_objhess *o, const double *free_,
                          double obj_factor, double *out, int32_t mem) {
    if (!o || !free_ || !out) return fail("null argument");
    if (mem != OPTY_HIP_HOST && mem != OPTY_HIP_DEVICE)
        return fail("bad memory kind %d", mem);
    HIP_TRY(hipSetDevice(o->d.device));
    // d_partial (and the staging buffers) may still be in use on the stream
    // the handle was on before opty_hip_objhess_set_stream
    if (int rc = order_streams(o)) return rc;
    const size_t nnz = (size_t)o->nnz();
    if (nnz == 0) return 0;         // nothing to write: nothing is launched
    const double *dfree = free_;
    double *dout = out;
    if (mem == OPTY_HIP_HOST) {
        if (int rc = ensure(&o->d_free, (size_t)o->num_free())) return rc;
        if (int rc = ensure(&o->d_out, nnz)) return rc;
        HIP_TRY(hipMemcpyAsync(o->d_free, free_, o->num_free()*sizeof(double),
                               hipMemcpyHostToDevice, o->stream));
        dfree = o->d_free;
        dout = o->d_out;
    }
    ObjHessArgs a{};
    a.free_ = dfree;
    a.partial = o->d_partial;
    a.out = dout;
    a.h = o->d.h;
    a.factor = obj_factor;
    a.N = o->d.N;
    a.nblk = o->nblk;
    size_t size = sizeof a;
    void *config[] = {HIP_LAUNCH_PARAM_BUFFER_POINTER, &a,
                      HIP_LAUNCH_PARAM_BUFFER_SIZE, &size,
                      HIP_LAUNCH_PARAM_END};
    HIP_TRY(hipModuleLaunchKernel(o->k_hess, (unsigned)o->nblk, 1, 1, 64, 1, 1,
                                  0, o->stream, nullptr, config));
    if (o->d.T > 0)
        HIP_TRY(hipModuleLaunchKernel(o->k_fin, 1, 1, 1, 64, 1, 1, 0,
                                      o->stream, nullptr, config));
    if (mem == OPTY_HIP_HOST) {
        HIP_TRY(hipMemcpyAsync(out, o->d_out, nnz*sizeof(double),
                               hipMemcpyDeviceToHost, o->stream));
        HIP_TRY(hipStreamSynchronize(sync_target(o->stream)));
    }
    return 0;
}

}  // extern "C"

// ---------------------------------------------------------------------------
// plain matrix functions (ufuncify_matrix call shape)
// ---------------------------------------------------------------------------
struct opty_hip_matrix {
    opty_hip_matrix_desc d{};
    hipModule_t module = nullptr;
    hipFunction_t k_mat = nullptr, k_uni = nullptr;
    hipStream_t own_stream = nullptr, stream = nullptr;
    hipStream_t last_stream = nullptr;   // stream of the last enqueued work
    double *d_args = nullptr, *d_result = nullptr, *d_const = nullptr,
           *d_uni = nullptr;
    size_t args_cap = 0, result_cap = 0;    // doubles
    std::vector<double> last_const;
    bool uni_valid = false;
};

namespace {

int grow(double **ptr, size_t *cap, size_t need) {
    if (need <= *cap) return 0;
    if (*ptr) HIP_TRY(hipFree(*ptr));
    *ptr = nullptr;
    *cap = 0;
    HIP_TRY(hipMalloc(reinterpret_cast<void **>(ptr), need*sizeof(double)));
    *cap = need;
    return 0;
}

}  // namespace

extern "C" {

int opty_hip_matrix_create(const opty_hip_matrix_desc *desc,
                           const char *code_object_path,
                           opty_hip_matrix **out) {
    if (!desc || !code_object_path || !out) return fail("null argument");
    if (desc->num_vec < 0 || desc->num_const < 0 || desc->rows < 1 ||
        desc->cols < 1)
        return fail("bad matrix shape %d x %d (%d vector, %d const args)",
                    desc->rows, desc->cols, desc->num_vec, desc->num_const);
    if (desc->wgs_per_block < 1 || desc->waves_per_wg < 1 ||
        desc->waves_per_wg > 16)
        return fail("bad launch geometry (%d workgroups x %d waves)",
                    desc->wgs_per_block, desc->waves_per_wg);
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count == 0)
        return fail("no HIP device is visible: the HIP backend has no CPU "
                    "fallback");
    if (desc->device < 0 || desc->device >= count)
        return fail("device %d out of range (have %d)", desc->device, count);
    HIP_TRY(hipSetDevice(desc->device));
    auto *m = new opty_hip_matrix;
    m->d = *desc;
    hipError_t e = hipModuleLoad(&m->module, code_object_path);
    if (e != hipSuccess) {
        delete m;
        (void)hipGetLastError();
        return fail("hipModuleLoad(%s) failed: %s", code_object_path,
                    hipGetErrorString(e));
    }
    if (hipModuleGetFunction(&m->k_mat, m->module, "opty_jac") != hipSuccess ||
        (desc->num_uniform > 0 &&
         hipModuleGetFunction(&m->k_uni, m->module, "opty_uni") !=
             hipSuccess)) {
        (void)hipModuleUnload(m->module);
        delete m;
        return fail("opty_jac/opty_uni missing from %s", code_object_path);
    }
    auto allocate = [&]() -> int {
        HIP_TRY(hipStreamCreateWithFlags(&m->own_stream,
                                         hipStreamNonBlocking));
        m->stream = m->own_stream;
        if (desc->num_const > 0)
            HIP_TRY(hipMalloc((void **)&m->d_const,
                              desc->num_const*sizeof(double)));
        if (desc->num_uniform > 0)
            HIP_TRY(hipMalloc((void **)&m->d_uni,
                              desc->num_uniform*sizeof(double)));
        return 0;
    };
    if (int rc = allocate()) {
        (void)opty_hip_matrix_destroy(m);
        return rc;
    }
    *out = m;
    return 0;
}

int opty_hip_matrix_destroy(opty_hip_matrix *m) {
    if (!m) return 0;
    (void)hipSetDevice(m->d.device);
    if (m->stream) (void)hipStreamSynchronize(sync_target(m->stream));
    void *bufs[] = {m->d_args, m->d_result, m->d_const, m->d_uni};
    for (void *b : bufs)
        if (b) (void)hipFree(b);
    if (m->own_stream) (void)hipStreamDestroy(m->own_stream);
    if (m->module) (void)hipModuleUnload(m->module);
    delete m;
    return 0;
}

int opty_hip_matrix_set_stream(opty_hip_matrix *m, void *hip_stream) {
    if (!m) return fail("null handle");
    m->stream = hip_stream ? (hipStream_t)hip_stream : m->own_stream;
    return 0;
}

int opty_hip_matrix_eval(opty_hip_matrix *m, double *result,
                         const double *const *vec_args,
                         const double *const_args, int64_t n, int32_t mem) {
    if (!m || !result) return fail("null argument");
    if (n < 1) return fail("need at least one evaluation row, got %lld",
                           (long long)n);
    if (m->d.num_vec > 0 && !vec_args) return fail("null vector arguments");
    if (m->d.num_const > 0 && !const_args)
        return fail("null const arguments");
    if (mem != OPTY_HIP_HOST && mem != OPTY_HIP_DEVICE)
        return fail("bad memory kind %d", mem);
    for (int k = 0; k < m->d.num_vec; ++k)
        if (!vec_args[k]) return fail("vector argument %d is null", k);
    HIP_TRY(hipSetDevice(m->d.device));
    // the packed arguments, the const table and the node-invariant table may
    // still be in use on the stream the handle was on before
    // opty_hip_matrix_set_stream
    if (int rc = order_streams(m)) return rc;
    const size_t size = (size_t)m->d.rows*m->d.cols;
    // the kernel reads the vector arguments as the rows of ONE (num_vec, n)
    // array (what `free` is to the collocation kernels): pack them
    if (int rc = grow(&m->d_args, &m->args_cap,
                      (size_t)std::max(1, m->d.num_vec)*n)) return rc;
    const hipMemcpyKind in = mem == OPTY_HIP_HOST ? hipMemcpyHostToDevice
                                                  : hipMemcpyDeviceToDevice;
    for (int k = 0; k < m->d.num_vec; ++k)
        HIP_TRY(hipMemcpyAsync(m->d_args + (size_t)k*n, vec_args[k],
                               n*sizeof(double), in, m->stream));
    // const arguments: by value in the reference; the table of
    // sub-expressions that depend on them alone is refilled when they change
    bool changed = !m->uni_valid ||
                   m->last_const.size() != (size_t)m->d.num_const;
    for (int k = 0; !changed && k < m->d.num_const; ++k)
        changed = std::memcmp(&m->last_const[k], &const_args[k],
                              sizeof(double)) != 0;
    double *out = result;
    if (mem == OPTY_HIP_HOST) {
        if (int rc = grow(&m->d_result, &m->result_cap, size*n)) return rc;
        out = m->d_result;
    }
    KernelArgs a{};
    a.free_ = m->d_args;
    a.params = m->d_const;
    a.uni_c = m->d_uni;
    a.uni_w = m->d_uni;
    a.jac = out;
    a.h = 1.0;
    a.N = n;
    a.con_stride = n;
    a.node_begin = 0;
    a.node_end = n;
    size_t asize = sizeof a;
    void *config[] = {HIP_LAUNCH_PARAM_BUFFER_POINTER, &a,
                      HIP_LAUNCH_PARAM_BUFFER_SIZE, &asize,
                      HIP_LAUNCH_PARAM_END};
    if (changed) {
        if (m->d.num_const > 0) {
            // pageable source: the copy has consumed it when the call returns
            HIP_TRY(hipMemcpyAsync(m->d_const, const_args,
                                   m->d.num_const*sizeof(double),
                                   hipMemcpyHostToDevice, m->stream));
            m->last_const.assign(const_args, const_args + m->d.num_const);
        }
        if (m->d.num_uniform > 0)
            HIP_TRY(hipModuleLaunchKernel(m->k_uni, OPTY_UNI_WORKGROUPS, 1, 1,
                                          64, 1, 1, 0, m->stream, nullptr,
                                          config));
        m->uni_valid = true;
    }
    const long long nblk = ((n + 63)/64 + 7)/8*8;
    HIP_TRY(hipModuleLaunchKernel(m->k_mat,
                                  (unsigned)(nblk*m->d.wgs_per_block), 1, 1,
                                  64*m->d.waves_per_wg, 1, 1, 0, m->stream,
                                  nullptr, config));
    if (mem == OPTY_HIP_HOST) {
        HIP_TRY(hipMemcpyAsync(result, out, size*n*sizeof(double),
                               hipMemcpyDeviceToHost, m->stream));
        HIP_TRY(hipStreamSynchronize(sync_target(m->stream)));
    }
    return 0;
}


}  // extern "C"
