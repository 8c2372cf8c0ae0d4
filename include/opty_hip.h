/* opty_hip.h -- C ABI of libopty_hip.so, the MI355X-native replacement for the
 * native code opty generates at run time for its direct-collocation hot path.
 *
 * What it replaces in the reference (csu-hmc/opty, paths relative to the
 * reference root):
 *
 *   - the generated per-node C function  `void eval_matrix(double matrix[R*C],
 *     double a0, ...)` (template opty/utils.py:483-498) and its Cython node
 *     loop `eval_matrix_loop` (opty/utils.py:500-529), instantiated twice per
 *     problem by ConstraintCollocator._gen_multi_arg_con_func
 *     (opty/direct_collocation.py:2373-2378) and _gen_multi_arg_con_jac_func
 *     (opty/direct_collocation.py:2798-2803);
 *   - the free-vector unpacking and output re-layout around them
 *     (opty/direct_collocation.py:2382-2446, :2816-2887, :2928-3001), which is
 *     folded into the kernels: the library consumes `free` and produces the
 *     flat `constraints(free)` / `jacobian(free)` vectors directly;
 *   - ConstraintCollocator.jacobian_indices
 *     (opty/direct_collocation.py:2450-2690).
 *
 * The per-problem device code is a gfx950 code object (.hsaco) produced by
 * opty_amd.codegen (the counterpart of ufuncify_matrix, opty/utils.py:639-928)
 * that exports the kernels `opty_con`, `opty_jac`, `opty_conjac`, `opty_uni`
 * (node-invariant sub-expressions) and, when the problem has instance
 * constraints, `opty_inst`.
 *
 * All functions return 0 on success and a non-zero code on failure;
 * opty_hip_last_error() then holds a message (thread-local).  A handle is not
 * thread-safe (neither is the reference: opty/utils.py:548, :672-675).  There
 * is no CPU fallback: without a HIP device opty_hip_create fails.
 *
 * Layouts (identical to the reference's):
 *   free : [x_0[0..N-1] ... x_{n-1}[..], u_0[0..N-1] ... u_{q-1}[..],
 *           p_0..p_{r-1}, h]                 (opty/direct_collocation.py:116-125)
 *   con  : con[j*(N-1) + i] for equation j, constraint node i, then the o
 *           instance constraints            (opty/direct_collocation.py:2446)
 *   jac  : jac[i*P + j*C + k], P = M*C, then the instance partials
 *                                           (opty/direct_collocation.py:2885-2887)
 *   rows/cols : int64 COO indices of every jac entry, same order
 *                                           (opty/direct_collocation.py:2628-2688)
 */
#ifndef OPTY_HIP_H
#define OPTY_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct opty_hip_problem opty_hip_problem;

enum { OPTY_HIP_BACKWARD_EULER = 0, OPTY_HIP_MIDPOINT = 1 };
/* where the caller's `free` / output buffers live */
enum { OPTY_HIP_HOST = 0, OPTY_HIP_DEVICE = 1 };
/* selector for opty_hip_time_eval */
enum { OPTY_HIP_EVAL_CON = 0, OPTY_HIP_EVAL_JAC = 1, OPTY_HIP_EVAL_PAIR = 2,
       OPTY_HIP_EVAL_FUSED = 3,
       /* the fused kernel itself, whatever opty_hip_desc.fused_loses says
        * (measurement tools) */
       OPTY_HIP_EVAL_FUSED_KERNEL = 4 };

/* opty_hip_desc.routing.
 * CALIBRATE: at the first OPTY_HIP_EVAL_FUSED / OPTY_HIP_EVAL_JAC launch of
 *   every launch size the handle times opty_conjac, opty_con and opty_jac on
 *   its own device (hipEvents, a few launches into the caller's buffers) and
 *   from then on launches the faster of fused kernel / pair and of opty_jac /
 *   fused kernel; desc.fused_loses / desc.jac_via_fused (the launch plan's
 *   flags, measured on the tuner's box) only break ties (1 %).
 *   OPTY_HIP_ROUTING=plan in the environment keeps the flags as they are.
 * NO_JAC_KERNEL / NO_FUSED_KERNEL: that kernel of the module must never be
 *   launched (the build found it to spill vector registers):
 *   EVAL_JAC and the pair go through the fused kernel / EVAL_FUSED issues
 *   opty_con + opty_jac.  Not both. */
#define OPTY_HIP_ROUTE_CALIBRATE 1
#define OPTY_HIP_ROUTE_NO_JAC_KERNEL 2
#define OPTY_HIP_ROUTE_NO_FUSED_KERNEL 4

#define OPTY_HIP_LAYOUT_COO 0
#define OPTY_HIP_LAYOUT_CSR 1
#define OPTY_HIP_LAYOUT_SEGMENTED 2

/* strip classes a list schedule can hold (opty_hip_desc.jac_class_cost) */
#define OPTY_HIP_MAX_CLASSES 32

typedef struct opty_hip_desc {
    int64_t N;            /* collocation (time) nodes                        */
    int32_t n;            /* states                                          */
    int32_t M;            /* equations of motion                             */
    int32_t m_known;      /* known input trajectories                        */
    int32_t q;            /* unknown input trajectories                      */
    int32_t p_known;      /* known parameters                                */
    int32_t r;            /* unknown parameters                              */
    int32_t s;            /* 1 if the node time interval is free             */
    int32_t C;            /* columns of the per-node block (len(wrt))        */
    int32_t P;            /* values stored per node: M*C (the reference's dense
                             block), fewer when structural zeros are pruned  */
    int32_t method;       /* OPTY_HIP_BACKWARD_EULER / OPTY_HIP_MIDPOINT     */
    int32_t num_inst;     /* o: instance constraints                         */
    int32_t nnz_inst;     /* instance-constraint Jacobian entries            */
    int32_t num_inst_atoms; /* distinct x(t_k) atoms in instance constraints */
    int32_t jac_wgs_per_block; /* workgroups per 64-node block (opty_jac)    */
    int32_t jac_waves_per_wg;  /* 64-lane waves per such workgroup           */
    int32_t fused_wgs_per_block; /* workgroups per block of opty_conjac      */
    int32_t con_wgs_per_block; /* workgroups per block of opty_con           */
    int32_t num_uniform;  /* entries of the node-invariant table (opty_uni)  */
    int32_t uniform_dynamic; /* 1 if that table depends on `free` (r+s > 0)  */
    int32_t device;       /* HIP device ordinal                              */
    int32_t fused_waves_per_wg; /* waves per workgroup of opty_conjac         */
    int32_t con_waves_per_wg;   /* waves per workgroup of opty_con            */
    int32_t layout;       /* OPTY_HIP_LAYOUT_COO: the reference's node-major
                             order jac[i*P + e]; OPTY_HIP_LAYOUT_CSR: sorted by
                             row then column, jac[S_j*(N-1) + i*L_j + pos]
                             (needs opty_hip_set_block_pattern);
                             OPTY_HIP_LAYOUT_SEGMENTED: the block's entries in
                             three node-major segments, jac[S_g*(N-1) + i*L_g
                             + pos] (needs opty_hip_set_segments)            */
    int32_t inst_folded;  /* 1: opty_con / opty_jac / opty_conjac evaluate the
                             instance tails themselves when launched with one
                             workgroup more than the node blocks need (small
                             problems: saves the launch of opty_inst)        */
    int32_t fused_loses;  /* 1: for this problem and launch size the fused
                             kernel was MEASURED slower than opty_con followed
                             by opty_jac (launch plan): opty_hip_eval_con_jac
                             and OPTY_HIP_EVAL_FUSED issue the two launches.
                             The reference evaluates the two callbacks
                             separately in any case
                             (opty/direct_collocation.py:498-562)            */
    int32_t jac_via_fused; /* 1: the launch plan measured opty_conjac FASTER than
                             opty_jac for this problem and launch size (the
                             constraint waves ride in the shadow of the store
                             stream): OPTY_HIP_EVAL_JAC launches the fused
                             kernel, its constraint values go to a scratch
                             vector of the handle                            */
    int32_t jac_persist;  /* > 0: opty_jac is a persistent kernel with a list
                             schedule: launched with at most this many
                             one-wave workgroups (a multiple of 8; 1024 = one
                             per SIMD), each of which evaluates a list of
                             (node block, strip class) items that the library
                             computes per launch size -- longest class first
                             onto the least loaded workgroup of the block's
                             XCD -- from the class costs below.  A launch of
                             waves that each hold a SIMD alone then costs
                             about sum(wave durations) / 1024, without the idle
                             time a one-wave-per-item dispatch leaves between
                             and after the waves                              */
    int32_t fused_persist; /* the same for opty_conjac                        */
    int32_t routing;      /* OPTY_HIP_ROUTE_* bits: which of the module's
                             kernels the entry points may launch, and whether
                             the handle measures the choice itself           */
    float jac_class_cost[OPTY_HIP_MAX_CLASSES];   /* relative duration of the
                             wave of strip class g (any unit; measured by the
                             launch plan's tuner or the printer's estimate);
                             classes = jac_wgs_per_block                      */
    float fused_class_cost[OPTY_HIP_MAX_CLASSES];
    int32_t var_jac_wgs_per_block; /* > 0: the module carries the RESTRICTED
                             flavour of the Jacobian kernels, opty_jac_var and
                             opty_conjac_var, which write only the 128-byte
                             lines of a block that hold an entry that can
                             change between two evaluations (see
                             opty_hip_output_register); workgroups per
                             64-node block of opty_jac_var.  0: no such
                             kernels (nothing worth skipping, another layout,
                             or a build that spilled): registration is
                             accepted and has no effect                       */
    int32_t var_jac_waves_per_wg;  /* waves per such workgroup                */
    int32_t var_fused_wgs_per_block; /* the same for opty_conjac_var          */
    int32_t var_fused_waves_per_wg;
} opty_hip_desc;

/* Version of this header's structs and signatures; opty_hip_abi_version()
 * returns the one the library was built from.  A client built against another
 * version must not call the library: the descriptor grew in 5, 6, 7 and 8
 * (8: the restricted kernels' geometry, opty_hip_output_*; 9: the
 * opty_hip_jacprod_* entry points; 10: the opty_hip_objhess_* entry points;
 * 11: the opty_hip_hessmv_* entry points; 12: opty_hip_hessmv_apply_block
 * and opty_hip_hessmv_block_width; the opty_hip_jacprod_block_* entry points
 * came later WITHOUT a new version: they are purely additive, no struct or
 * signature of version 12 changed, and a client finds out whether its library
 * has them by looking the symbols up; likewise, later still,
 * opty_hip_jacprod_jvp_shard / opty_hip_jacprod_jvp_instance /
 * opty_hip_jacprod_vjp_shard, and then opty_hip_eval_hess_shard /
 * opty_hip_eval_hess_instance / opty_hip_hessian_indices_range, and then the
 * opty_hip_hesscsr_* entry points, and then
 * opty_hip_hesscsr_create_with_diagonal and the opty_hip_kktcsr_* entry
 * points, and then opty_hip_hessmv_apply_shard, and then the
 * opty_hip_normal_* entry points), and
 * opty_hip_eval_jac_persistent / opty_hip_shard_jac_to_host took their `fresh`
 * argument in 4. */
#define OPTY_HIP_ABI_VERSION 12
int opty_hip_abi_version(void);

/* (The build verification's device side -- register poisoner, instruction
 * tape -- is a library of its own: include/opty_hip_referee.h.) */

/* The list schedule the library gives a persistent kernel (opty_hip_desc.
 * jac_persist / fused_persist) for a launch over `node_blocks` 64-node blocks
 * with `classes` strip classes of relative duration class_cost[g]: host
 * arithmetic only (inspection, tests).  table[0] = workgroups npw;
 * table[1 .. npw + 1] = first item of workgroup w (workgroup w serves XCD
 * w % 8); table[npw + 2 ...] = items, (class << 24) | s for node block
 * 8 s + XCD, every workgroup's in the order in which it evaluates them.
 * `table` may be null (count only). */
int opty_hip_list_schedule(int persist, int64_t node_blocks, int classes,
                           const float *class_cost, int32_t *table,
                           int64_t capacity, int64_t *count);

/* The run schedule of a restricted kernel in run form
 * (opty_hip_set_restricted_runs), in the same table format: per XCD the items
 * in (block slot, class) order -- a block's classes adjacent -- cut into
 * persist/8 CONTIGUOUS runs whose summed class costs are within one largest
 * item of their mean.  Host arithmetic only. */
int opty_hip_run_schedule(int persist, int64_t node_blocks, int classes,
                          const float *class_cost, int32_t *table,
                          int64_t capacity, int64_t *count);

/* Loads the code object and allocates the device-side state (known
 * parameters, known trajectories, staging buffers). */
int opty_hip_create(const opty_hip_desc *desc, const char *code_object_path,
                    opty_hip_problem **out);
int opty_hip_destroy(opty_hip_problem *p);

/* Replaces the handle's restricted kernels by their RUN form, which lives in
 * a code object of its own (`code_object_path`; the handle's module keeps the
 * dispatch form, one workgroup per block and strip, and its other kernels are
 * what they are without this call): opty_jac_var is launched with at most
 * `jac_persist` one-wave workgroups (a multiple of 8), each of which walks a
 * contiguous run of (node block, strip class) items (opty_hip_run_schedule)
 * and fills the slab / evaluates the block's sin and cos only where the block
 * changes; `jac_class_cost[g]`, g < jac_classes, is the relative duration of
 * strip class g (one workgroup per class and block in this form).  The same
 * for opty_conjac_var.  The code object must carry the global `opty_run_form`
 * and both kernels: anything else is refused, so neither form can be launched
 * as the other.  Once per handle; a handle without the call evaluates
 * registered outputs with the dispatch form.  (An entry point of its own:
 * the descriptor is unchanged.) */
int opty_hip_set_restricted_runs(opty_hip_problem *p,
                                 const char *code_object_path,
                                 int jac_persist, int jac_classes,
                                 const float *jac_class_cost,
                                 int fused_persist, int fused_classes,
                                 const float *fused_class_cost);

/* The null / legacy default stream (hipStreamLegacy) as a set_stream argument:
 * NULL itself means "the handle's own stream". */
#define OPTY_HIP_STREAM_LEGACY ((void *)1)

/* Use an existing hipStream_t (e.g. torch's current stream; pass
 * OPTY_HIP_STREAM_LEGACY for the default stream, whose handle is NULL) for
 * all work of this handle; NULL restores the handle's own stream.  A handle's device
 * state belongs to one stream at a time: the first evaluation after a switch
 * waits (on the host) for everything the handle enqueued on the previous
 * stream. */
int opty_hip_set_stream(opty_hip_problem *p, void *hip_stream);
int opty_hip_synchronize(opty_hip_problem *p);

/* Values of the known parameters in ConstraintCollocator.known_parameters
 * order.  Replaces the scalar by-value arguments c0.. of eval_matrix
 * (opty/utils.py:489-490) that _multi_arg_con_func passes on every call
 * (opty/direct_collocation.py:2436-2437). */
int opty_hip_set_known_parameters(opty_hip_problem *p, const double *values,
                                  int32_t count);
/* Node time interval when it is not a free variable; must be set before the
 * first evaluation (the reference passes `interval_value` per call,
 * opty/direct_collocation.py:2382-2385, :2437). */
int opty_hip_set_interval(opty_hip_problem *p, double h);
/* (m_known x N) row-major array, known_input_trajectories order: the known
 * rows _merge_fixed_free interleaves into the specifieds
 * (opty/direct_collocation.py:2891-2926). */
int opty_hip_set_known_trajectories(opty_hip_problem *p, const double *values,
                                    int32_t mem);
/* Instance constraints: free-vector index of every atom
 * (_find_closest_free_index, opty/direct_collocation.py:2169-2217) and the COO
 * rows/cols of the instance part of the Jacobian
 * (_instance_constraints_jacobian_indices, :2233-2251); host arrays. */
int opty_hip_set_instance_indices(opty_hip_problem *p,
                                  const int64_t *atom_free_index,
                                  const int64_t *rows, const int64_t *cols);

/* Pruned blocks (P < M*C) and the CSR layout: (j, k) of every stored entry
 * of a block in storage order, 2*P int32 (CSR: grouped by j, ascending
 * column within a row). */
int opty_hip_set_block_pattern(opty_hip_problem *p, const int32_t *jk);

int64_t opty_hip_num_free(const opty_hip_problem *p);
int64_t opty_hip_num_constraints(const opty_hip_problem *p);
int64_t opty_hip_nnz(const opty_hip_problem *p);

/* constraints(free): writes num_constraints doubles.  Replaces the closure
 * built by _wrap_constraint_funcs(..., 'con') (opty/direct_collocation.py:
 * 2952-2993) including _multi_arg_con_func (:2382-2446) and the compiled
 * eval_matrix_loop (opty/utils.py:500-529). */
int opty_hip_eval_con(opty_hip_problem *p, const double *free, double *con,
                      int32_t mem);
/* jacobian(free): writes nnz doubles.  Replaces the 'jac' closure of
 * _wrap_constraint_funcs and _multi_arg_con_jac_func
 * (opty/direct_collocation.py:2816-2887). */
int opty_hip_eval_jac(opty_hip_problem *p, const double *free, double *jac,
                      int32_t mem);
/* both of the above for one `free` from one kernel launch (no reference
 * counterpart: IPOPT asks for them separately, :498-525, :552-562). */
int opty_hip_eval_con_jac(opty_hip_problem *p, const double *free, double *con,
                          double *jac, int32_t mem);
/* ---- host-visible Jacobian: only what changed crosses PCIe ------------------
 * The reference returns jacobian(free) in ONE persistent array that the next
 * call overwrites (opty/direct_collocation.py:2814, :2885-2887) and whose
 * per-node block is dense -- structural zeros and node-invariant entries
 * included (:2589-2593).  opty_hip_set_varying_entries names the block entries
 * whose value can differ between two evaluations with the same known
 * parameters and node time interval (ascending, 0 <= e < P; everything else
 * is a function of those alone: literal zeros, +-1, 1/h, masses ...).
 * opty_hip_eval_jac_persistent(free, jac), both HOST, jac page-locked
 * (opty_hip_host_alloc), then computes the same values as opty_hip_eval_jac
 * but moves only the varying entries -- packed on the device, copied in chunks,
 * scattered into `jac` by a pool of host threads -- whenever `jac` is the
 * vector of the previous call and the invariant entries it holds are still
 * valid (they are re-sent after opty_hip_set_known_parameters /
 * opty_hip_set_interval).  The caller must not write into `jac` between
 * calls, and passes `fresh` != 0 on the FIRST call with an allocation (and
 * whenever it may have written into it): the library compares addresses only
 * as a second line of defence -- an allocator hands a freed block out again at
 * the same address, so address identity is not a validity token.  Node-major
 * layout only; without varying entries set it is opty_hip_eval_jac. */
int opty_hip_set_varying_entries(opty_hip_problem *p, const int32_t *entries,
                                 int32_t count);
/* Block entries that are the SAME expression as an earlier varying entry (a
 * symmetric mass matrix; its entries in the columns of the current and of the
 * adjacent node's speeds): they are not named as varying entries, do not cross
 * PCIe, and the host threads fill entry dst[k] of every node's block from
 * entry src[k] of the same block (dst ascending and not varying entries; src
 * varying entries).  Call after opty_hip_set_varying_entries, which clears the
 * list. */
int opty_hip_set_entry_copies(opty_hip_problem *p, const int32_t *dst,
                              const int32_t *src, int32_t count);
/* The same with a factor per copy: the host threads fill entry dst[k] with
 * scale[k] x entry src[k] of the same block -- varying entries that are a
 * node-invariant multiple of another varying entry (c_1 X and c_2 X over the
 * same per-node expression X: scale = c_1/c_2, computed by the caller from the
 * known parameters and set again when those change) do not cross PCIe either.
 * scale == NULL: plain copies.  A factor of exactly 1.0 reproduces the source
 * bit for bit. */
int opty_hip_set_entry_copies_scaled(opty_hip_problem *p, const int32_t *dst,
                                     const int32_t *src, const double *scale,
                                     int32_t count);
int opty_hip_eval_jac_persistent(opty_hip_problem *p, const double *free,
                                 double *jac, int32_t fresh);
/* ---- OPTY_HIP_LAYOUT_SEGMENTED: a host-visible Jacobian without a scatter ---
 * IPOPT takes the (row, col, value) triplets in any order
 * (opty/direct_collocation.py:527-562 hands it rows / cols once, :552-562 the
 * values per call).  In this layout the dense block of the reference
 * (:2589-2593) is stored as three node-major segments,
 *
 *   jac = [ seg 0 of node 0 .. N-2 | seg 1 of node 0 .. N-2 | seg 2 ... | tail ]
 *
 * order[0 .. P): the block entries (reference numbering e = j*C + k) in
 * stored order -- seg_len[0] entries that can differ between two evaluations,
 * then seg_len[1] entries that are the same expression as an entry of segment
 * 0 (copy_source[k]: its position in segment 0), then seg_len[2] entries that
 * depend on known parameters and the node time interval alone.  The kernels
 * and opty_hip_jacobian_indices follow that order; HOST evaluations move
 * segment 0 over PCIe straight into the head of the caller's vector, fill
 * segment 1 on the host from it, and -- opty_hip_eval_jac_persistent -- leave
 * segment 2 alone after the first call (re-sent after
 * opty_hip_set_known_parameters / opty_hip_set_interval and when `fresh`).
 * No read-for-ownership of the dense vector, no per-entry scatter.  Whole
 * problems only (node shards use the node-major layout). */
int opty_hip_set_segments(opty_hip_problem *p, const int32_t *order,
                          const int32_t *seg_len, const int32_t *copy_source);
/* Largest fraction of a block's stored entries for which only the varying
 * ones are moved (beyond it whole blocks are copied and no entry copies are
 * applied): 0.8, or OPTY_HIP_PACK_RATIO. */
double opty_hip_pack_ratio(void);
/* Where the host threads that scatter the varying entries run (NUMA node, -1:
 * unplaced), the NUMA node of the current device, and whether the placement
 * has been verified by measurement (the pool times its candidates when a
 * scatter ends late; OPTY_HIP_HOST_PLACEMENT=fixed disables that). */
int opty_hip_host_placement(int32_t *workers_node, int32_t *device_node,
                            int32_t *verified);
/* The same for one node shard of a problem evaluated by several GPUs: the
 * blocks of the constraint nodes [node_begin, node_end), as
 * opty_hip_eval_shard left them in device memory (d_jac_shard), go into the
 * slice [node_begin*P, node_end*P) of the dense HOST vector of the GLOBAL
 * problem (host_jac: the shared page-locked vector every rank copies its
 * shard into, SURVEY.md 8(e) "direct-to-host") -- all of them the first
 * time (and whenever `fresh` != 0: a new mapping of the shared vector, see
 * above), later only the varying entries.  Synchronous; runs on the handle's
 * stream behind the evaluation. */
int opty_hip_shard_jac_to_host(opty_hip_problem *p, const double *d_jac_shard,
                               double *host_jac, int64_t node_begin,
                               int64_t node_end, int32_t fresh);
/* Host threads of the scatter pool (per process; 0 = the default:
 * OPTY_HIP_HOST_THREADS, or min(16, hardware threads / 4 / LOCAL_WORLD_SIZE)
 * -- the ranks of a node share the cores of the NUMA node that holds the one
 * vector they all scatter into; each worker gets a core of its own there,
 * LOCAL_RANK deciding which).  The workers run on the cores of
 * the NUMA node that holds the caller's dense vector (get_mempolicy);
 * OPTY_HIP_HOST_NUMA=<node> overrides, =off leaves them where the creating
 * thread may run.  The workers never leave the affinity mask of the thread
 * that created the pool (taskset / cpuset / an OpenMP binding are honoured,
 * and the pool has at most as many workers as that mask has CPUs);
 * OPTY_HIP_HOST_AFFINITY=wide lifts that for applications whose binding pins
 * only the calling thread. */
int opty_hip_set_host_threads(int32_t count);
int opty_hip_host_threads(void);
/* NUMA node that holds the first page of a host allocation (-1: unknown). */
int opty_hip_host_numa_node(const void *ptr);

/* jacobian_indices(): writes nnz int64 rows and cols -- the closed form of
 * ConstraintCollocator.jacobian_indices (opty/direct_collocation.py:2450-2690,
 * formulas :2644-2675). */
int opty_hip_jacobian_indices(opty_hip_problem *p, int64_t *rows,
                              int64_t *cols, int32_t mem);

/* The same for a handle that evaluates the constraint nodes
 * [node_offset, node_offset + N - 1) of a larger problem with N_global nodes
 * (node sharding across GPUs): global row/col indices of the shard's values. */
int opty_hip_jacobian_indices_shard(opty_hip_problem *p, int64_t N_global,
                                    int64_t node_offset, int64_t *rows,
                                    int64_t *cols, int32_t mem);

/* Global indices of the values opty_hip_eval_shard writes for the constraint
 * nodes [node_begin, node_end) of this handle's problem: (node_end -
 * node_begin)*P int64 each. */
int opty_hip_jacobian_indices_range(opty_hip_problem *p, int64_t node_begin,
                                    int64_t node_end, int64_t *rows,
                                    int64_t *cols, int32_t mem);

/* Runs `iters` evaluations back to back on the handle's stream with device
 * buffers and returns the mean milliseconds per evaluation measured with
 * hipEvents recorded on that stream. */
int opty_hip_time_eval(opty_hip_problem *p, int32_t what, const double *free,
                       double *con, double *jac, int32_t iters,
                       float *ms_per_iter);

/* ---- node shards (one process per GPU) ----------------------
 * Evaluates the constraint nodes [node_begin, node_end) of the handle's
 * problem from the GLOBAL free vector (device memory, full length; only the
 * time-node columns [node_begin, node_end] of its trajectory rows and its
 * parameter tail contribute -- the one-node halo of
 * opty/direct_collocation.py:2411-2413; the last 64-node block may touch up
 * to 64 columns past node_end, whose values are not used).
 * Device pointers only:
 *   con : the shard's value of equation j, node i goes to
 *         con[j*con_stride + (i - node_begin)]; con_stride = N-1 with
 *         con = global_con + node_begin writes the shard in place into the
 *         global equation-major vector (opty/direct_collocation.py:2446),
 *         con_stride = node_end - node_begin gives a dense (M x nodes) block;
 *   jac : the shard's blocks, jac[(i - node_begin)*P + e]; jac =
 *         global_jac + node_begin*P is the contiguous slice
 *         [node_begin*P, node_end*P) of the global node-major vector
 *         (opty/direct_collocation.py:2885-2887).
 * `what` is OPTY_HIP_EVAL_*.  Shards cover the collocation part only: the
 * instance constraints of a problem that has them are evaluated once, by
 * whichever rank assembles the vectors, with opty_hip_eval_instance.  The CSR
 * layout is not sharded. */
int opty_hip_eval_shard(opty_hip_problem *p, int32_t what, const double *free,
                        double *con, int64_t con_stride, double *jac,
                        int64_t node_begin, int64_t node_end);
/* The instance-constraint tails from the GLOBAL free vector (device
 * pointers): the o values that follow the M*(N-1) collocation constraints
 * (opty/direct_collocation.py:2985-2991) into con_tail[0..o) and the nnz_inst
 * partials that follow the P*(N-1) block values (:2686-2688, :2253-2282) into
 * jac_tail[0..nnz_inst); either may be NULL.  What a rank of a node-sharded
 * problem calls for the tail of the vector it assembles; a no-op for problems
 * without instance constraints. */
int opty_hip_eval_instance(opty_hip_problem *p, const double *free,
                           double *con_tail, double *jac_tail);
/* opty_hip_time_eval for a shard. */
int opty_hip_time_eval_shard(opty_hip_problem *p, int32_t what,
                             const double *free, double *con,
                             int64_t con_stride, double *jac,
                             int64_t node_begin, int64_t node_end,
                             int32_t iters, float *ms_per_iter);

/* Registered device outputs.  The OWNER of a device Jacobian buffer that
 * keeps what the library wrote into it -- nobody else writes to it between two
 * evaluations -- says so: opty_hip_output_register(p, jac, node_begin,
 * node_end) for the buffer that opty_hip_eval_shard (or, with the whole node
 * range [0, N-1), opty_hip_eval_jac / opty_hip_eval_con_jac with device
 * memory) is given for that node range.  Two thirds of a multibody block are
 * the same at every node and every call (structural zeros, +-1, +-1/h,
 * products of known masses and lengths): the first evaluation into a
 * registered buffer writes everything, the following ones launch the module's
 * restricted kernels (opty_hip_desc.var_*), which write only the 128-byte
 * lines that hold an entry that can change; the bytes in between are NOT
 * touched, so the buffer is read-only for its owner between calls.  Everything
 * is written again after whatever can change a node-invariant entry or leaves
 * the buffer's contents in doubt: opty_hip_set_known_parameters,
 * opty_hip_set_interval, opty_hip_set_block_pattern, opty_hip_set_segments, a
 * reload of the module, an evaluation of ANOTHER node range into the buffer,
 * an evaluation that returned an error, opty_hip_output_invalidate (jac ==
 * NULL: every registered buffer of the handle; what an owner calls after
 * writing to the buffer itself).  The registration is the owner's word: the
 * library never infers persistence from an address it has seen before, and an
 * unregistered pointer is always written whole.  Unregister before the memory
 * is released.  OPTY_HIP_DENSE_OUTPUT=1 in the environment (read once) turns
 * the restricted path off: registered buffers are written whole, too.
 * Registering a registered address again replaces its node range;
 * unregistering or invalidating an address that is not registered is an
 * error.  At most 64 buffers per handle. */
int opty_hip_output_register(opty_hip_problem *p, double *jac,
                             int64_t node_begin, int64_t node_end);
int opty_hip_output_unregister(opty_hip_problem *p, double *jac);
int opty_hip_output_invalidate(opty_hip_problem *p, double *jac);

/* What the entry points launch for a launch of `node_count` constraint nodes
 * (opty_hip_desc.routing): bit 0 of *calibrated is set when the handle has
 * measured that launch size on its device (ms3[0..2] = per-launch ms of
 * opty_conjac, opty_con, opty_jac as measured), clear when the launch plan's
 * flags are still in force; bit 1 is set when the LAST Jacobian launch of
 * that size was served by the restricted flavour (opty_conjac_var /
 * opty_jac_var into a registered output) -- the flags and times are then
 * that flavour's, which is calibrated on its own; *fused_loses = 1: OPTY_HIP_EVAL_FUSED issues opty_con + opty_jac;
 * *jac_via_fused = 1: OPTY_HIP_EVAL_JAC launches opty_conjac.  Any output
 * pointer may be null.  The reference calls its two callbacks separately
 * (opty/direct_collocation.py:498-562): whichever kernel serves them, the
 * values are those of the same expressions. */
int opty_hip_routing(opty_hip_problem *p, int64_t node_count,
                     int32_t *calibrated, int32_t *fused_loses,
                     int32_t *jac_via_fused, float *ms3);

/* ---- objective and objective gradient -------------
 * Device counterpart of create_objective_function (opty/utils.py:329-470):
 * value = h*sum_i w_i G(node i) + b(p) and its gradient with respect to
 * free = [x rows, u rows, p], quadrature weights per opty/utils.py:419-464.
 * The code object exports `opty_objgrad` and `opty_objfin`. */
typedef struct opty_hip_objective opty_hip_objective;

typedef struct opty_hip_objective_desc {
    int64_t N;        /* collocation nodes                                   */
    int32_t n, q, r;  /* states, unknown inputs, unknown parameters          */
    int32_t device;   /* HIP device ordinal                                  */
    double h;         /* node time interval                                  */
} opty_hip_objective_desc;

int opty_hip_objective_create(const opty_hip_objective_desc *desc,
                              const char *code_object_path,
                              opty_hip_objective **out);
int opty_hip_objective_destroy(opty_hip_objective *o);
int opty_hip_objective_set_stream(opty_hip_objective *o, void *hip_stream);
/* value: one double (host memory, always); grad: (n+q)*N + r doubles in `mem`
 * memory or NULL for the value alone; free: (n+q)*N + r doubles in `mem`. */
int opty_hip_objective_eval(opty_hip_objective *o, const double *free,
                            double *value, double *grad, int32_t mem);

/* ---- exact Hessian of the objective -----------------------------------------
 * H = d2 f / d free^2 of the value f that opty_hip_objective_eval returns,
 * for the objectives it supports, sum_j a_j(p) Integral(g_j, t) + b(p) with
 * G = sum_j a_j g_j:
 *   backward Euler: f = h sum_{i=1}^{N-1} G(z_i, p) + b(p)  (H is then also the
 *                   Jacobian of the gradient opty_hip_objective_eval returns)
 *   midpoint:       f = h sum_{i=0}^{N-2} G((z_i + z_{i+1})/2, p) + b(p)  (the
 *                   reference-shaped midpoint gradient evaluates its trajectory
 *                   part at the node values and is not the gradient of f: H is
 *                   the Hessian of the VALUE)
 * Contract of the constraint Hessian below: lower triangle (row >= col on the
 * GLOBAL free indices), triplets, a (row, col) pair may repeat and the matrix
 * is the SUM of its triplets.  Both methods have N-1 quadrature points; point
 * j is node j + base (base = 1 backward Euler, 0 midpoint).
 *   out : out[e*(N-1) + j] for per-point entry e < E and point j, then the T
 *         parameter-parameter entries out[E*(N-1) + t] = h sum_j G_pp + b_pp;
 *         every value times obj_factor.  nnz = E*(N-1) + T may be 0.
 * The code object exports `opty_objhess` (lane = quadrature point) and, when
 * T > 0, `opty_objhess_fin` (one wave: block partials added in a fixed
 * order).  No atomics: every value is written exactly once per call and the
 * same inputs give the same bits.  Nothing is launched when nnz == 0. */
typedef struct opty_hip_objhess opty_hip_objhess;

typedef struct opty_hip_objhess_desc {
    int64_t N;        /* collocation nodes                                   */
    int32_t n, q, r;  /* states, unknown inputs, unknown parameters          */
    int32_t device;   /* HIP device ordinal                                  */
    double h;         /* node time interval                                  */
    int32_t base;     /* node of quadrature point 0: 1 backward Euler, 0 mid */
    int32_t E;        /* per-point entries                                   */
    int32_t T;        /* parameter-parameter entries                         */
} opty_hip_objhess_desc;

/* pattern (host memory, copied): 4 int32 per per-point entry e, (row_var,
 * row_off, col_var, col_off) -- global index of a side = var*N + j + base +
 * off for var >= 0 (off 0, or 1 with base 0), (n+q)*N + off for var == -1
 * (parameter off) -- then 2 int32 per parameter-parameter entry, the
 * parameters (a, b) of its row and column.  May be null when E == T == 0. */
int opty_hip_objhess_create(const opty_hip_objhess_desc *desc,
                            const int32_t *pattern,
                            const char *code_object_path,
                            opty_hip_objhess **out);
int opty_hip_objhess_destroy(opty_hip_objhess *o);
int opty_hip_objhess_set_stream(opty_hip_objhess *o, void *hip_stream);
/* E*(N-1) + T */
int64_t opty_hip_objhess_nnz(const opty_hip_objhess *o);
/* int64 row / column indices of every value, same order, in `mem` memory. */
int opty_hip_objhess_indices(opty_hip_objhess *o, int64_t *rows,
                             int64_t *cols, int32_t mem);
/* free: (n+q)*N + r doubles, out: nnz doubles, both in `mem` memory.
 * Synchronous for OPTY_HIP_HOST (staged through buffers of the handle);
 * OPTY_HIP_DEVICE writes straight to `out` -- which may point into a larger
 * buffer, a double's alignment is enough -- and is enqueued on the handle's
 * stream. */
int opty_hip_objhess_eval(opty_hip_objhess *o, const double *free,
                          double obj_factor, double *out, int32_t mem);

/* ---- plain matrix functions: the reference's plugin call shape ---------------
 * `f = ufuncify_matrix(args, expr, const=...)`, `f(result, *num_args)`
 * (opty/utils.py:639-640; argument contract :610-617, :778-807): a rows x cols
 * matrix of expressions evaluated for n independent argument rows, the
 * generated `eval_matrix` + `eval_matrix_loop` pair (opty/utils.py:483-529)
 * as one gfx950 kernel (`opty_jac` of a "matrix program", lane = evaluation
 * row, row-major (n, rows*cols) output through the same tile flush as a
 * Jacobian block) plus `opty_uni` for sub-expressions of the const
 * arguments alone. */
typedef struct opty_hip_matrix opty_hip_matrix;

typedef struct opty_hip_matrix_desc {
    int32_t num_vec;        /* vector arguments: one double per row           */
    int32_t num_const;      /* const arguments: one double per call           */
    int32_t rows, cols;     /* shape of the matrix                            */
    int32_t wgs_per_block;  /* launch geometry of opty_jac (from the emitter) */
    int32_t waves_per_wg;
    int32_t num_uniform;    /* entries of the node-invariant table            */
    int32_t device;         /* HIP device ordinal                             */
} opty_hip_matrix_desc;

int opty_hip_matrix_create(const opty_hip_matrix_desc *desc,
                           const char *code_object_path,
                           opty_hip_matrix **out);
int opty_hip_matrix_destroy(opty_hip_matrix *m);
int opty_hip_matrix_set_stream(opty_hip_matrix *m, void *hip_stream);
/* result: n*rows*cols doubles, result[i*rows*cols + r*cols + c];
 * vec_args: HOST array of num_vec pointers, each to n contiguous doubles in
 * `mem` memory (n >= 1); const_args: num_const doubles in HOST memory (passed
 * by value in the reference).  Synchronous for OPTY_HIP_HOST, enqueued on the
 * handle's stream for OPTY_HIP_DEVICE. */
int opty_hip_matrix_eval(opty_hip_matrix *m, double *result,
                         const double *const *vec_args,
                         const double *const_args, int64_t n, int32_t mem);

/* Page-locked host memory for OPTY_HIP_HOST callers: output arrays that live
 * in it (the persistent Jacobian value buffer the reference keeps,
 * opty/direct_collocation.py:2814) are copied back at full PCIe rate. */
void *opty_hip_host_alloc(size_t bytes);
int opty_hip_host_free(void *ptr);
/* Page-locks memory the caller already owns -- e.g. a shared-memory mapping
 * of the one host vector that IPOPT reads and into which every rank copies its
 * node shard over its own PCIe link ("direct-to-host"). */
int opty_hip_host_register(void *ptr, size_t bytes);
int opty_hip_host_unregister(void *ptr);
/* Device memory for callers without a HIP toolchain of their own (a plain C
 * host that node-shards a problem: opty_hip_eval_shard and the communicator
 * calls below take device pointers); `kind`: 0 host->device, 1 device->host,
 * 2 device->device, synchronous. */
void *opty_hip_device_alloc(int32_t device, size_t bytes);
int opty_hip_device_free(void *ptr);
int opty_hip_memcpy(void *dst, const void *src, size_t bytes, int32_t kind);

/* ---------------------------------------------------------------------------
 * Several GPUs, one process each: the RCCL side of a node-sharded problem
 * (BASELINE config 4).  The reference parallelises the node
 * loop over an OpenMP team (opty/utils.py:524-526); here every rank evaluates
 * its node range with opty_hip_eval_shard from the global free vector in its
 * own HBM, and these calls move (i) that vector to every rank and (ii) the
 * shards to a rank that wants whole vectors -- RCCL point-to-point over xGMI
 * on the problem handle's stream, issued by this library (librccl is loaded
 * on first use).  No call here is needed on a single GPU.
 *
 * Bring-up: rank 0 calls opty_hip_comm_unique_id and hands the
 * OPTY_HIP_COMM_ID_BYTES bytes to the other ranks by whatever means the
 * launcher offers (a file, MPI, a torch.distributed store); every rank then
 * calls opty_hip_comm_create (collective: it returns when all `world` ranks
 * have called it). */
typedef struct opty_hip_comm opty_hip_comm;
#define OPTY_HIP_COMM_ID_BYTES 128
int opty_hip_comm_unique_id(void *id_out /* OPTY_HIP_COMM_ID_BYTES bytes */);
int opty_hip_comm_create(const void *unique_id, int32_t rank, int32_t world,
                         int32_t device, opty_hip_comm **out);
int opty_hip_comm_destroy(opty_hip_comm *c);
int opty_hip_comm_rank(const opty_hip_comm *c);
int opty_hip_comm_world(const opty_hip_comm *c);
/* Broadcast of the global free vector (device memory, opty_hip_num_free
 * doubles on every rank) from rank `root`, ordered on `p`'s stream like an
 * evaluation.  A no-op in a world of one. */
int opty_hip_bcast_free(opty_hip_comm *c, opty_hip_problem *p,
                        double *free_dev, int32_t root);
/* Gather-v of node shards to rank `root`.  `bounds`: world + 1 ascending
 * constraint-node boundaries, rank g owns [bounds[g], bounds[g+1]) (shards
 * may differ in size and may be empty).  Every other rank passes what
 * opty_hip_eval_shard wrote for its range: `jac_shard` = its (b-a)*P values,
 * `con_shard` = its dense (M, b-a) block (con_stride = b-a); one grouped
 * ncclSend each.  The root passes the global vectors of the problem
 * (opty_hip_num_constraints / opty_hip_nnz doubles): the peers' Jacobian
 * slices are received IN PLACE (jac[a*P .. b*P), contiguous in the node-major
 * layout, opty/direct_collocation.py:2885-2887), their constraint blocks into
 * staging that one strided device copy per peer puts at con[j*(N-1) + a]
 * (equation-major, :2446).  The root's own shard is copied from `con_shard` /
 * `jac_shard` unless those are NULL (it evaluated in place: con_stride = N-1,
 * jac + a*P).  `what`: OPTY_HIP_EVAL_CON, _JAC or _PAIR (both).  The o
 * instance constraints are not node shards: the root evaluates them itself
 * (opty_hip_eval_instance).  Asynchronous on `p`'s stream. */
int opty_hip_gather_v(opty_hip_comm *c, opty_hip_problem *p,
                      const int64_t *bounds, const double *con_shard,
                      const double *jac_shard, double *con_global,
                      double *jac_global, int32_t root, int32_t what);

/* ---- exact Hessian of the constraint Lagrangian ------------------------------
 * hess = sum_k lagrange_k * (second derivatives of constraint k) with respect
 * to `free`, lower triangle (row >= col on the GLOBAL free indices), as
 * triplets.  lagrange is ordered like `con`: lagrange[j*(N-1) + i], then the o
 * instance constraints.  A (row, col) pair REPEATS: the matrix is the SUM of
 * its triplets (IPOPT's and scipy.sparse.coo_matrix's convention) -- a time
 * node's diagonal block gets a term from both constraint nodes that share it,
 * a parameter / h entry one from every node.
 *   hess : hess[i*PH + e] for constraint node i and per-node entry e, then the
 *          nnz_inst entries of the instance constraints.
 * The code object exports `opty_hess` (lane = constraint node; grid.y = the
 * `strips` pieces of a node's PH entries) and, when nnz_inst > 0,
 * `opty_hess_inst`.
 *
 * A Hessian handle BORROWS its problem handle: device, stream, known
 * parameters, known trajectories, the fixed node time interval and the
 * instance atom indices are the problem's own (one copy; what a set_known
 * call installs is seen by the next Hessian call).  It must be destroyed
 * before the problem handle. */
typedef struct opty_hip_hessian opty_hip_hessian;

typedef struct opty_hip_hessian_desc {
    int32_t PH;        /* stored entries per constraint node                   */
    int32_t nnz_inst;  /* entries of the instance constraints                  */
    int32_t strips;    /* workgroups per 64-node block of opty_hess            */
    /* closed-form index pattern, 4 int32 per per-node entry e:
     * (row_a, off_a, row_b, off_b); global index of a side = row*N + i + off
     * for row >= 0, (n+q)*N + off for row == -1 (parameter / h tail) */
    const int32_t *pattern;
    const int64_t *inst_rows;   /* nnz_inst global indices each (host memory) */
    const int64_t *inst_cols;
} opty_hip_hessian_desc;

int opty_hip_hessian_create(opty_hip_problem *p,
                            const opty_hip_hessian_desc *desc,
                            const char *code_object_path,
                            opty_hip_hessian **out);
int opty_hip_hessian_destroy(opty_hip_hessian *h);
/* (N-1)*PH + nnz_inst */
int64_t opty_hip_hessian_nnz(const opty_hip_hessian *h);
/* free: num_free doubles, lagrange: num_constraints doubles, hess:
 * hessian_nnz doubles, all in `mem` memory.  Synchronous for OPTY_HIP_HOST,
 * enqueued on the problem's stream for OPTY_HIP_DEVICE.
 * OPTY_HIP_DEVICE with an even PH: `hess` must be 16-byte aligned (a node's
 * entries are written with 16-byte stores); a pointer that is not is refused
 * ("... must be 16-byte aligned ...") before anything is enqueued.  An odd PH
 * and OPTY_HIP_HOST need no more than a double's alignment. */
int opty_hip_eval_hess(opty_hip_hessian *h, const double *free,
                       const double *lagrange, double *hess, int32_t mem);
/* int64 row / column indices of every hess value, same order. */
int opty_hip_hessian_indices(opty_hip_hessian *h, int64_t *rows,
                             int64_t *cols, int32_t mem);

/* ---- node-sharded Hessian: a window of the constraint nodes -------------------
 * What opty_hip_jacprod_jvp_shard is to J v: the values of the constraint
 * nodes [node_begin, node_end) of the handle's GLOBAL problem, for a host that
 * node-shards one problem over several GPUs.  Device pointers only, enqueued
 * on the problem's stream.  `free` and `lagrange` are the GLOBAL vectors at
 * full length (num_free resp. num_constraints doubles); the kernels are the
 * two above, opty_hess launched over the window.
 *   eval_hess_shard    : hess_shard[(i - node_begin)*PH + e] = hess[i*PH + e],
 *                        node i of the window: (node_end - node_begin)*PH
 *                        doubles.  hess_shard = global + node_begin*PH writes
 *                        in place.
 *   eval_hess_instance : the nnz_inst instance values hess[(N-1)*PH + t] into
 *                        inst_out; by whichever rank assembles the vector.
 *                        Succeeds and writes nothing when nnz_inst == 0.
 *   indices_range      : the global row / column indices of a window's values
 *                        ((node_end - node_begin)*PH each, in `mem` memory).
 * Contract: a node's entries depend on that node's inputs and multipliers
 * alone and the triplets ADD, so there is no halo node and no sum across
 * windows: every value of every window has the BITS of opty_hip_eval_hess,
 * for any partition, and nothing outside the window's slice is written.  An
 * empty window succeeds and launches nothing.  Refused before anything is
 * enqueued, with the offending number in opty_hip_last_error(): null
 * pointers, node_begin < 0, node_end > N-1, node_begin > node_end, and, when
 * PH is even, a hess_shard that is not 16-byte aligned (every in-place window
 * base is aligned whenever the global base is; an odd PH is written with
 * 8-byte stores and needs a double's alignment only). */
int opty_hip_eval_hess_shard(opty_hip_hessian *h, const double *free,
                             const double *lagrange, double *hess_shard,
                             int64_t node_begin, int64_t node_end);
int opty_hip_eval_hess_instance(opty_hip_hessian *h, const double *free,
                                const double *lagrange,
                                double *inst_out /* nnz_inst doubles */);
int opty_hip_hessian_indices_range(opty_hip_hessian *h, int64_t node_begin,
                                   int64_t node_end, int64_t *rows,
                                   int64_t *cols, int32_t mem);

/* ---- matrix-free Jacobian products ------------------------------------------
 * J is the matrix of opty_hip_jacobian_indices + opty_hip_eval_jac: shape
 * (num_constraints, num_free), the SUM of its triplets; the products do not
 * depend on the Jacobian's layout or pruning.
 *   jvp : out = J(free) v,   v of num_free doubles, out of num_constraints
 *         doubles ordered like `con` (j*(N-1) + i, then the o instance
 *         constraints);
 *   vjp : out = J(free)^T w, w of num_constraints doubles, out of num_free
 *         doubles ordered like `free`.
 * Nothing of the size of the matrix is read or written: a product reads
 * `free` and one vector and writes one vector.  Every entry of `out` is
 * written exactly once per call, in a fixed order of operations (no
 * floating-point atomics): the same inputs give the same bits.
 * The code object exports `opty_jvp` (grid.y = jvp_strips), `opty_jvp_inst`,
 * `opty_vjp` (blocks of 64 lanes that advance by 63 constraint nodes; grid.y
 * = vjp_strips) and `opty_vjp_fin`.
 *
 * A product handle BORROWS its problem handle exactly as a Hessian handle
 * does, and must be destroyed before it. */
typedef struct opty_hip_jacprod opty_hip_jacprod;

typedef struct opty_hip_jacprod_desc {
    int32_t jvp_strips; /* workgroups per 64-node block of opty_jvp            */
    int32_t vjp_strips; /* workgroups per 63-node block of opty_vjp            */
    int32_t num_tail;   /* r + s: tail entries of `free` (block partials)      */
    int32_t nnz_inst;   /* first partials of the instance constraints          */
} opty_hip_jacprod_desc;

int opty_hip_jacprod_create(opty_hip_problem *p,
                            const opty_hip_jacprod_desc *desc,
                            const char *code_object_path,
                            opty_hip_jacprod **out);
int opty_hip_jacprod_destroy(opty_hip_jacprod *h);
/* All three arrays in `mem` memory.  Synchronous for OPTY_HIP_HOST, enqueued
 * on the problem's stream for OPTY_HIP_DEVICE. */
int opty_hip_jacprod_jvp(opty_hip_jacprod *h, const double *free,
                         const double *v, double *out, int32_t mem);
int opty_hip_jacprod_vjp(opty_hip_jacprod *h, const double *free,
                         const double *w, double *out, int32_t mem);

/* ---- node-sharded products: a window of the constraint nodes ------------------
 * What opty_hip_eval_shard is to the evaluation: the products of the rows
 * (jvp) resp. onto the columns (vjp) that belong to the constraint nodes
 * [node_begin, node_end) of the handle's GLOBAL problem, for a host that
 * node-shards one problem over several GPUs.  Device pointers only, enqueued on
 * the problem's stream.  `free`, `v` and `w` are the GLOBAL vectors at full
 * length (num_free resp. num_constraints doubles); the kernels are the four
 * above, launched over the window.
 *   jvp_shard    : out[j*out_stride + (i - node_begin)] = (J v)[j*(N-1) + i],
 *                  equation j, node i of the window.  out_stride = N-1 with
 *                  out = global + node_begin writes in place, out_stride =
 *                  node_end - node_begin gives a dense (M, count) block.
 *   jvp_instance : the o instance rows (J v)[M*(N-1) + k] into out_tail; by
 *                  whichever rank assembles the vector.
 *   vjp_shard    : the window OWNS the time nodes p in [node_begin, node_end)
 *                  and, when node_end == N-1, also p = N-1.
 *                  out[R*out_stride + (p - node_begin)] = (J^T w)[R*N + p],
 *                  free row R, owned p, the instance constraints' terms of
 *                  the atoms at owned time nodes included.  out_stride = N
 *                  with out = global + node_begin writes in place, out_stride
 *                  = the number of owned nodes gives a dense block.
 *                  tail_part[t], t < r + s: the window's share of the tail
 *                  entry (J^T w)[(n+q)*N + t], the sum over the window's
 *                  constraint nodes; the entry is the sum of the shares of
 *                  the windows of a partition.  May be null when r + s == 0.
 * Contract: every entry of jvp_shard, and every entry of vjp_shard's `out`,
 * has the BITS of the whole-problem product (the same lane arithmetic, the
 * same two-term sum, the same instance additions in the same order), for any
 * partition; tail_part is deterministic per window, and for the window
 * [0, N-1) bit-identical to the whole product's tail.  Nothing outside the
 * window's slice of `out` is written.  An empty window succeeds, launches
 * nothing and zero-fills tail_part.  Refused before anything is enqueued:
 * null pointers, node_begin < 0, node_end > N-1, node_begin > node_end, an
 * out_stride below the window's width. */
int opty_hip_jacprod_jvp_shard(opty_hip_jacprod *h, const double *free,
                               const double *v, double *out,
                               int64_t out_stride, int64_t node_begin,
                               int64_t node_end);
int opty_hip_jacprod_jvp_instance(opty_hip_jacprod *h, const double *free,
                                  const double *v,
                                  double *out_tail /* o doubles */);
int opty_hip_jacprod_vjp_shard(opty_hip_jacprod *h, const double *free,
                               const double *w, double *out,
                               int64_t out_stride,
                               double *tail_part /* r + s doubles */,
                               int64_t node_begin, int64_t node_end);

/* ---- block products: Y = J(free) V and G = J(free)^T W ----------------------
 * The products above for `ncols` vectors in one call.  Column c of V is the
 * num_free doubles at V + c*ldv, of Y the num_constraints doubles at Y +
 * c*ldy; column c of W the num_constraints doubles at W + c*ldw, of G the
 * num_free doubles at G + c*ldg.  A leading dimension may exceed the column
 * length (interior blocks of a larger matrix): what lies between two result
 * columns is never written, nothing outside the columns is read.
 * The code object is a module of its own, generated for `width` (4 or 2)
 * columns per pass: `opty_jvp_block` (grid.y = jvp_strips),
 * `opty_jvp_block_inst`, `opty_vjp_block` (grid.y = vjp_strips) and
 * `opty_vjp_block_fin`, the geometry of the four single kernels.  What does
 * not depend on the column -- trig, the collected coefficients, the
 * mass-matrix factors -- is evaluated once per pass; a call makes
 * ceil(ncols/width) passes.  Every result element is written exactly once, in
 * a fixed order of operations: the same inputs give the same bits (not
 * necessarily those of the single products: the expressions are associated
 * differently).
 * Refused before anything is enqueued, each with the offending number: null
 * pointers, ncols < 0, a leading dimension below the column length, a result
 * range that overlaps `free` or the input block, a bad `mem`.  ncols == 0
 * succeeds and launches nothing.  OPTY_HIP_HOST: synchronous, the columns are
 * staged without their padding; OPTY_HIP_DEVICE: enqueued on the problem's
 * stream.  The handle BORROWS its problem handle as opty_hip_jacprod does. */
typedef struct opty_hip_jacprod_block opty_hip_jacprod_block;

typedef struct opty_hip_jacprod_block_desc {
    int32_t width;       /* K of the module: 2 or 4                            */
    int32_t jvp_strips;  /* workgroups per 64-node block of opty_jvp_block     */
    int32_t vjp_strips;  /* workgroups per 63-node block of opty_vjp_block     */
    int32_t num_tail;    /* r + s: tail entries of `free` (block partials)     */
    int32_t nnz_inst;    /* first partials of the instance constraints         */
} opty_hip_jacprod_block_desc;

int opty_hip_jacprod_block_create(opty_hip_problem *p,
                                  const opty_hip_jacprod_block_desc *desc,
                                  const char *code_object_path,
                                  opty_hip_jacprod_block **out);
int opty_hip_jacprod_block_destroy(opty_hip_jacprod_block *h);
/* Columns per pass (the descriptor's width); -1 for a null handle. */
int32_t opty_hip_jacprod_block_width(const opty_hip_jacprod_block *h);
int opty_hip_jacprod_block_jvp(opty_hip_jacprod_block *h, const double *free,
                               const double *V, int64_t ldv,
                               double *Y, int64_t ldy,
                               int32_t ncols, int32_t mem);
int opty_hip_jacprod_block_vjp(opty_hip_jacprod_block *h, const double *free,
                               const double *W, int64_t ldw,
                               double *G, int64_t ldg,
                               int32_t ncols, int32_t mem);

/* ---- Hessian operator: y = H v from the stored triplets ----------------------
 * H is the symmetric matrix whose LOWER triangle is the SUM of the triplets of
 * the Hessian of the Lagrangian: a triplet (r, c, a) adds a*v[c] to y[r] and,
 * when r != c, a*v[r] to y[c]; a diagonal triplet counts once.  `values` is
 * laid out as its pieces are evaluated, in this order:
 *   node section       values[i*PH + e], constraint node i (opty_hip_eval_hess;
 *                      `pattern` as in opty_hip_hessian_desc)
 *   instance entries   nnz_inst values, explicit (inst_rows, inst_cols)
 *   objective section  values[.. + e*(N-1) + j], quadrature point j
 *                      (opty_hip_objhess_eval; `obj_pattern`: (var_a, off_a,
 *                      var_b, off_b) per entry, free index var*N + j + obj_base
 *                      + off, or the tail entry (n+q)*N + off for var == -1);
 *                      E = T = 0: no objective section
 *   parameter-parameter entries   T values, explicit (tail_rows, tail_cols)
 * Relative to a node every side of an entry of either section is (row, slot),
 * slot in {0, 1}, or a tail entry; anything else is refused at creation, as
 * are explicit indices outside [0, num_free) or above the diagonal.
 *
 * One kernel family of this library serves every problem (no code object):
 * `opty_hessmv` (lane = node; blocks of 64 lanes that advance by 63 nodes; an
 * LDS accumulator per distinct side and lane) and `opty_hessmv_fin` (one wave:
 * the tail entries from the block partials, in block order, then the explicit
 * triplets in stored order by one lane; launched only when the problem has
 * tail entries or explicit triplets).  Every element of y is stored exactly
 * once by opty_hessmv or by opty_hessmv_fin's last loop -- rows that no triplet
 * touches get 0.0 --, in a fixed order of operations and without atomics: the
 * same inputs give the same bits in every call and for both memory kinds.
 * The distinct sides must fit the LDS of one block (1 KiB per side next to a
 * 16.5 KiB tile); a pattern with more is refused at creation with a message
 * that names the count and the limit.
 *
 * Block products Y = H V over several columns: `opty_hessmv_block<K>`, K = 2,
 * 3, 4, keeps K values of v and K accumulators per side and lane (16 896 +
 * 1 024*K*sides bytes of LDS), reads every value once for the K columns and
 * applies, per column, the operations of `opty_hessmv` in its order;
 * `opty_hessmv_block_fin` is `opty_hessmv_fin` with one block per column.  A
 * handle's pass width is the largest of 4, 3, 2 whose LDS fits the device's
 * limit per block, else 1; a call runs ceil(ncols / width) passes, the last one
 * as wide as what is left (one column: the single kernels).
 *
 * The handle BORROWS its problem handle for N, n, q, r, s, device and stream
 * (it reads none of the problem's tables) and must be destroyed before it. */
typedef struct opty_hip_hessmv opty_hip_hessmv;

typedef struct opty_hip_hessmv_desc {
    int32_t PH;        /* stored entries per constraint node                   */
    int32_t nnz_inst;  /* entries of the instance constraints                  */
    int32_t E;         /* objective entries per quadrature point               */
    int32_t obj_base;  /* 1: backward Euler, 0: midpoint                       */
    int32_t T;         /* parameter-parameter entries of the objective         */
    const int32_t *pattern;      /* 4*PH   (host memory, as all tables here)   */
    const int64_t *inst_rows;    /* nnz_inst global indices each               */
    const int64_t *inst_cols;
    const int32_t *obj_pattern;  /* 4*E                                        */
    const int64_t *tail_rows;    /* T global indices each                      */
    const int64_t *tail_cols;
} opty_hip_hessmv_desc;

int opty_hip_hessmv_create(opty_hip_problem *p,
                           const opty_hip_hessmv_desc *desc,
                           opty_hip_hessmv **out);
int opty_hip_hessmv_destroy(opty_hip_hessmv *h);
/* PH*(N-1) + nnz_inst + E*(N-1) + T */
int64_t opty_hip_hessmv_nnz(const opty_hip_hessmv *h);
/* The side table: returns the number of distinct sides, stores the number of
 * trajectory sides (they come first, ascending (row, slot); the tail sides
 * follow, ascending offset) and up to `room` (row, slot) pairs -- (-1, offset)
 * for a tail side.  `sides` and `num_trajectory` may be NULL. */
int32_t opty_hip_hessmv_sides(const opty_hip_hessmv *h, int32_t *sides,
                              int32_t room, int32_t *num_trajectory);
/* values: hessmv_nnz doubles (8-byte alignment is enough), v and y: num_free
 * doubles, all in `mem` memory; y must not overlap v or values.  Synchronous
 * for OPTY_HIP_HOST, enqueued on the problem's stream for OPTY_HIP_DEVICE. */
int opty_hip_hessmv_apply(opty_hip_hessmv *h, const double *values,
                          const double *v, double *y, int32_t mem);
/* Columns are contiguous vectors: column c of V at V + c*ldv, of Y at Y + c*ldy,
 * ldv, ldy >= num_free.  Column c of Y equals, bit for bit, what
 * opty_hip_hessmv_apply gives for column c of V; what lies between two columns
 * of Y is not written.  Memory kinds and ordering as for opty_hip_hessmv_apply;
 * ncols == 0 succeeds and launches nothing.  Refused before anything is
 * enqueued: null pointers, ncols < 0, ldv or ldy below num_free, a range of Y
 * that overlaps V or values. */
int opty_hip_hessmv_apply_block(opty_hip_hessmv *h, const double *values,
                                const double *V, int64_t ldv,
                                double *Y, int64_t ldy,
                                int32_t ncols, int32_t mem);
/* columns one pass takes (1 .. 4), fixed at create from the LDS the side table needs */
int32_t opty_hip_hessmv_block_width(const opty_hip_hessmv *h);

/* ---- Hessian operator over a node window (shards that stay in device memory) --
 * What opty_hip_jacprod_vjp_shard is to J^T w: the share of y = H v of the
 * constraint nodes [node_begin, node_end), from the GLOBAL v (num_free doubles)
 * and the values of those nodes where opty_hip_eval_hess_shard left them.  The
 * handle is one of the constraint section alone (E == 0 and T == 0: the
 * objective section is not node-sharded).
 *   values_shard : values_shard[(i - i_first)*PH + e], i_first = node_begin -
 *                  (node_begin > 0): entry p of a trajectory row needs node p - 1
 *                  too, so a window that does not start the problem holds one
 *                  (halo) node in front; 8-byte alignment is enough
 *   inst_values  : the nnz_inst instance values (opty_hip_eval_hess_instance)
 *   out          : the window OWNS the time nodes p in [node_begin, pend), pend =
 *                  node_end + (node_end == N - 1): out[R*out_stride + p -
 *                  node_begin] is entry R*N + p of y, out_stride >= pend -
 *                  node_begin; the instance triplets' sides at owned entries
 *                  included, in stored order
 *   tail_part    : r + s doubles by tail offset: the window's share of the
 *                  node-invariant entries -- the sum over its nodes, block
 *                  partials in block order; an entry without a side is 0.0 --
 *                  and, for the ONE call of a partition with tail_owner != 0, on
 *                  top of it the instance triplets' tail sides.  The entries
 *                  themselves are the sum of the windows' shares.
 * Contract: every entry of `out` has the bits of opty_hip_hessmv_apply on the
 * same handle and the whole problem's values, for every partition of the nodes;
 * tail_part has the same bits from call to call, and for the window [0, N - 1)
 * with tail_owner the bits of the whole product's tail; for other partitions it
 * is the same sum cut differently.  Nothing but the owned entries of `out` and
 * tail_part is written.  Device pointers only; enqueued on the problem's
 * stream, not synchronised.  Refused before anything is enqueued: null pointers
 * (inst_values may be NULL when nnz_inst == 0, tail_part when r + s == 0), a
 * window outside [0, N - 1] or with node_begin > node_end, an out_stride below
 * the owned width, a range of `out` that overlaps v or values_shard, a handle
 * with an objective section.  An empty window zero-fills tail_part and -- when
 * it owns the tail and the handle has instance triplets -- runs opty_hessmv_fin
 * alone; otherwise it launches nothing. */
int opty_hip_hessmv_apply_shard(opty_hip_hessmv *h,
                                const double *values_shard,
                                const double *inst_values, const double *v,
                                double *out, int64_t out_stride,
                                double *tail_part, int64_t node_begin,
                                int64_t node_end, int32_t tail_owner);

/* ---- Hessian as CSR: unique lower triangle, duplicates summed ------------------
 * The triplets of the Hessian of the Lagrangian -- `values` laid out as for the
 * Hessian operator above, the descriptor is its descriptor -- compressed to
 * the CSR lower triangle over num_free rows: exactly the distinct (row, col)
 * pairs, rows ascending, columns ascending within a row, a row without a
 * triplet empty; data[u] is the sum of the triplets of pair u.
 * scipy.sparse.csr_matrix((data, indices, indptr)) needs no conversion.
 *
 * The structure depends on the descriptor and N only and is closed form
 * (hessian_csr_structure of opty_amd/codegen/program.py is the host
 * statement): trajectory row R*N + p is the merge of the node entries of row
 * side (R, 0) at node p and of (R, 1) at node p - 1, the same L_R columns at
 * every interior time node; a tail row is one segment of consecutive time nodes
 * per trajectory row it couples with, then its tail columns; an explicit
 * triplet falls on a pair of the pattern or adds a column to its row.
 *
 * Kernels (this library's, no code object): `opty_hesscsr` -- lane = time node,
 * one wave per block, blocks of 64 lanes that advance by 63 nodes; the node
 * entries of a trajectory row class are a window of consecutive entries, and
 * the window of a group of consecutive classes (up to 64 entries, or the widest
 * class's) goes through an LDS tile for the block's 64 nodes; the outputs of a
 * class leave through a 64 x 33 tile, rows that follow one another in data as
 * one run; a segment is one coalesced store per lane -- and `opty_hesscsr_fin` -- lane =
 * item: the first and the last time node of every trajectory row, every row
 * with an explicit triplet, the tail x tail pairs, each with its list of
 * positions in `values`; launched when there are items.
 *
 * ORDER OF ADDITION.  A SHORT group -- every pair but a tail x tail pair with a
 * triplet per constraint node -- adds its triplets in ascending position in
 * `values`, starting from +0.0: the bits of np.add.at(zeros, slot, values).  A
 * LONG group: per node its triplets in ascending position from +0.0; lanes past
 * the last node and lane 0 of every block but the first (the repeated node)
 * count as 0.0; per block the tree x[l] += x[l + d] for d = 32, 16 .. 1; the
 * block partials in block order from +0.0; then the explicit triplets of the
 * pair in stored order.  The order depends on N alone: the same bits in every
 * call and for both memory kinds.  Every element of data is stored exactly
 * once, without atomics; nothing outside data is written.
 *
 * Creation refuses what opty_hip_hessmv_create refuses, a pattern entry above
 * the diagonal, 2^31 or more triplets, and a pattern in which the node entries
 * of one row class span so many consecutive entries that the tile (8*(64*(W|1)
 * + 64*33 + 64) bytes, W = max(64, widest class)) exceeds the LDS of a block,
 * with the count and the limit in the message.  The handle BORROWS its problem handle (N, n, q, r, s, device,
 * stream) and must be destroyed before it. */
typedef struct opty_hip_hesscsr opty_hip_hesscsr;

int opty_hip_hesscsr_create(opty_hip_problem *p,
                            const opty_hip_hessmv_desc *desc,
                            opty_hip_hesscsr **out);
int opty_hip_hesscsr_destroy(opty_hip_hesscsr *h);
/* input triplets: PH*(N-1) + nnz_inst + E*(N-1) + T */
int64_t opty_hip_hesscsr_nnz(const opty_hip_hesscsr *h);
/* distinct (row, col) pairs: the length of indices and of data */
int64_t opty_hip_hesscsr_nnz_unique(const opty_hip_hesscsr *h);
/* indptr: num_free + 1, indices: nnz_unique int64 values in `mem` memory;
 * synchronous for both memory kinds. */
int opty_hip_hesscsr_structure(opty_hip_hesscsr *h, int64_t *indptr,
                               int64_t *indices, int32_t mem);
/* values: hesscsr_nnz doubles (8-byte alignment is enough), data: nnz_unique
 * doubles, both in `mem` memory.  Synchronous for OPTY_HIP_HOST, enqueued on the
 * problem's stream for OPTY_HIP_DEVICE.  Refused before anything is enqueued:
 * null pointers, a data range that overlaps values, a bad memory kind. */
int opty_hip_hesscsr_compress(opty_hip_hesscsr *h, const double *values,
                              double *data, int32_t mem);

/* The same handle with EVERY diagonal pair stored, last in its row, whether or
 * not a triplet lands on it: an empty source list for (R, 0) in every
 * trajectory row class, in every whole row that items own and in every tail
 * row; a pair without a triplet is stored as +0.0 by the same kernels.
 * Everything else (arguments, refusals, the other entry points, the order of
 * addition) is opty_hip_hesscsr_create's. */
int opty_hip_hesscsr_create_with_diagonal(opty_hip_problem *p,
                                          const opty_hip_hessmv_desc *desc,
                                          opty_hip_hesscsr **out);

/* ---- Augmented system as CSR ---------------------------------------------------
 * The lower triangle of the interior-point augmented system
 *
 *     K = [[ W + diag(sigma) + delta_w I ,  J^T        ],
 *          [ J                           ,  -delta_c I ]]
 *     W = obj_factor d2f + sum_k lagrange_k d2c_k
 *
 * over n + m rows (n = num_free, m = num_constraints) as one CSR matrix with
 * int64 indptr (n + m + 1 entries) and indices: rows and columns ascend, every
 * pair is stored once (scipy: has_canonical_format), EVERY diagonal is stored
 * and is the last entry of its row -- delta_w and delta_c change between two
 * factorisations without a new structure.  The structure depends on the
 * descriptor, the block pattern, the instance indices and N only
 * (kkt_csr_structure of opty_amd/codegen/program.py is the host statement).
 *
 *   row r < n:  the columns of row r of the CSR Hessian above, and the
 *       diagonal (r, r) whether or not a triplet lands on it.
 *   row n + k:  the columns of row k of the CSR Jacobian (OPTY_HIP_LAYOUT_CSR:
 *       rows j*(N-1) + i, then the instance constraints), then the diagonal
 *       (n + k, n + k).  Row (j, i) holds L_j + 1 values and starts at
 *       nnz_hessian + (S_j + j)*(N-1) + i*(L_j + 1).
 *
 * Values.  An off-diagonal entry of the W block has the bits of the matching
 * element of opty_hip_hesscsr_compress (the same order of addition).  A
 * diagonal of the W block is (h + sigma_r) + delta_w, rounded in that order,
 * h the compressed element or +0.0 where no triplet lands, sigma_r +0.0
 * when sigma is NULL.  A Jacobian entry has the bits of jac_values at its
 * position.  A diagonal of the constraint block is 0.0 - delta_c.  Every
 * element of data is stored exactly once (a W diagonal by the compression,
 * then updated in place), without atomics; nothing outside data and the
 * handle's staging buffers is written; the same inputs give the same bits in
 * every call and for both memory kinds.
 *
 * Kernels (this library's): opty_hesscsr / opty_hesscsr_fin write the W part
 * straight into data[0 .. nnz_hessian); `opty_kkt_diag` -- lane = free row, one
 * index read per row --, `opty_kkt_jrows` -- the destination spans of the
 * equations swept flat in tiles of 2048 doubles, 16-byte stores counted from a
 * 16-byte boundary, one launch with a capped grid -- and `opty_kkt_inst` -- lane
 * = stored value of the instance rows -- follow on the problem's stream.
 *
 * Creation refuses, before a device is touched, a problem handle whose layout
 * is not OPTY_HIP_LAYOUT_CSR, a block pattern or instance indices that were
 * never set, columns of an equation that do not ascend and an instance tail
 * that is not sorted by row, then column; then what
 * opty_hip_hesscsr_create refuses.  All positions are 64-bit: only the
 * Hessian's triplets are held to fewer than 2^31.  Before anything is
 * uploaded, every span is checked to stay inside data.  The handle BORROWS its
 * problem handle and must be destroyed before it. */
typedef struct opty_hip_kktcsr opty_hip_kktcsr;

int opty_hip_kktcsr_create(opty_hip_problem *p,
                           const opty_hip_hessmv_desc *desc,
                           opty_hip_kktcsr **out);
int opty_hip_kktcsr_destroy(opty_hip_kktcsr *h);
/* stored values of K: the length of indices and of data */
int64_t opty_hip_kktcsr_nnz(const opty_hip_kktcsr *h);
/* stored values of the W block (diagonals included): data[0 .. nnz_hessian) */
int64_t opty_hip_kktcsr_nnz_hessian(const opty_hip_kktcsr *h);
/* the Hessian's triplets: the length of hess_values */
int64_t opty_hip_kktcsr_nnz_triplets(const opty_hip_kktcsr *h);
/* indptr: n + m + 1, indices: kktcsr_nnz int64 values in `mem` memory;
 * synchronous for both memory kinds. */
int opty_hip_kktcsr_structure(opty_hip_kktcsr *h, int64_t *indptr,
                              int64_t *indices, int32_t mem);
/* hess_values: kktcsr_nnz_triplets doubles laid out as for the Hessian
 * operator; jac_values: opty_hip_nnz doubles in the CSR layout; sigma: num_free
 * doubles or NULL; data: kktcsr_nnz doubles; all in `mem` memory, 8-byte
 * alignment is enough.  Synchronous for OPTY_HIP_HOST (staged through buffers
 * of the handle), enqueued on the problem's stream for OPTY_HIP_DEVICE.
 * Refused before anything is enqueued: null hess_values / jac_values / data,
 * a data range that overlaps an input, a bad memory kind. */
int opty_hip_kktcsr_assemble(opty_hip_kktcsr *h, const double *hess_values,
                             const double *jac_values, const double *sigma,
                             double delta_w, double delta_c, double *data,
                             int32_t mem);
/* The same for OPTY_HIP_DEVICE pointers, synchronous, with device events
 * around its four stages (measurements): stage_ms[0 .. 4) = milliseconds of
 * the compression (opty_hesscsr + opty_hesscsr_fin), opty_kkt_diag,
 * opty_kkt_jrows, opty_kkt_inst. */
int opty_hip_kktcsr_assemble_timed(opty_hip_kktcsr *h,
                                   const double *hess_values,
                                   const double *jac_values,
                                   const double *sigma, double delta_w,
                                   double delta_c, double *data,
                                   float *stage_ms);

/* ---- Normal matrix: a direct solve with the block-tridiagonal J D^-1 J^T ----
 *
 *     S = Jc[:, :T] diag(1/d[:T]) Jc[:, :T]^T + delta_c I
 *
 * Jc: the M(N-1) collocation rows of the constraint Jacobian, T = (n+q)N the
 * trajectory part of `free`.  Constraint node i touches only the time nodes i
 * and i + 1, so, ordered by node, S is symmetric block tridiagonal: N - 1
 * diagonal blocks A_i (M x M, row-major) and N - 2 couplings B_i = S[i+1, i].
 * With G_i the block of constraint node i (a structurally pruned entry is 0):
 *
 *   A_i[a,b] = sum_k G_i[a,k] G_i[b,k] / d[row_k*N + i + off_k]
 *              (+ delta_c when a == b), over the trajectory columns k in
 *              ascending (row, off);
 *   B_i[a,b] = sum_row G_{i+1}[a,k0(row)] G_i[b,k1(row)] / d[row*N + i + 1],
 *              over the free rows that have an offset-0 column k0 and an
 *              offset-1 column k1 (backward Euler: the unknown inputs have no
 *              offset-0 column and drop out).
 *
 * The tail columns (unknown parameters, a free interval) and the instance
 * rows are NOT part of S: S is all of J D^-1 J^T only for a problem that has
 * neither; otherwise it is a preconditioner (a low-rank correction for the
 * tail is not done).  Every element is one chain of fma over the columns in
 * the order above, the second factor divided by d first.
 *
 * Factorisation: block cyclic reduction with Cholesky factors of the
 * eliminated diagonal blocks (normal_factor / normal_solve of
 * opty_amd/codegen/program.py are the host statement): level l has n_l rows,
 * n_0 = N - 1, n_{l+1} = ceil(n_l/2); rows 1, 3, 5, ... are eliminated, rows
 * 0, 2, 4, ... survive as e = k/2; a level with one row is a plain Cholesky.
 * No pivoting; backward stable for a positive definite S.  A pivot that is
 * not positive and finite is replaced by 1 and recorded: the factorisation
 * runs to its end, opty_hip_normal_factor_status names the smallest (level,
 * row) that met one, and opty_hip_normal_solve refuses until a factorisation
 * succeeds.  That is a numerical status, never a device fault.
 *
 * The handle owns all level storage (about 4 M^2 doubles per constraint node
 * over all levels, plus three vectors per level):
 * opty_hip_normal_workspace_bytes.  Creation refuses an M whose three M x (M|1)
 * tiles of doubles exceed the LDS one block may use (82 with 160 KiB) and
 * names the limit; opty_hip_normal_max_equations returns it.  The same inputs
 * give the same bits in every call and for both memory kinds; nothing outside
 * the handle's buffers and the outputs is written.  The handle BORROWS its
 * problem handle (sizes, method, device, stream) and must be destroyed before
 * it. */
typedef struct opty_hip_normal_desc {
    int32_t M;            /* rows of a block: equations of motion              */
    int32_t P;            /* values stored per constraint node                 */
    int32_t layout;       /* OPTY_HIP_LAYOUT_COO: jac[i*P + e]; OPTY_HIP_LAYOUT_CSR:
                             jac[S_j*(N-1) + i*L_j + (e - S_j)], the entries
                             grouped by equation, ascending                    */
    const int32_t *pattern; /* (j, k) of every stored entry of a block in
                             storage order, 2*P int32: equation, wrt column
                             (of the problem handle's C)                       */
} opty_hip_normal_desc;

typedef struct opty_hip_normal opty_hip_normal;

int opty_hip_normal_create(opty_hip_problem *p,
                           const opty_hip_normal_desc *desc,
                           opty_hip_normal **out);
int opty_hip_normal_destroy(opty_hip_normal *h);
/* device memory the handle owns for the levels and its tables */
int64_t opty_hip_normal_workspace_bytes(const opty_hip_normal *h);
/* the largest M creation accepts on the handle's device */
int32_t opty_hip_normal_max_equations(const opty_hip_normal *h);
/* jac_values: the P*(N-1) block values in the descriptor's layout (what
 * follows them is not read); d: (n+q)*N doubles, positive (not checked), or
 * NULL for all ones; A: (N-1)*M*M, B: (N-2)*M*M doubles (may be NULL when N ==
 * 2); all in `mem` memory.  Synchronous for OPTY_HIP_HOST, enqueued on the
 * problem's stream for OPTY_HIP_DEVICE.  Does not touch a factorisation.
 * Refused before anything is enqueued: null pointers, a bad memory kind,
 * delta_c < 0 or not finite, outputs that overlap an input or each other. */
int opty_hip_normal_blocks(opty_hip_normal *h, const double *jac_values,
                           const double *d, double delta_c, double *A,
                           double *B, int32_t mem);
/* Forms the blocks in the handle's storage and factorises them there. */
int opty_hip_normal_factor(opty_hip_normal *h, const double *jac_values,
                           const double *d, double delta_c, int32_t mem);
/* Waits for the last factorisation: *level = -1 when every pivot was positive
 * and finite, else the smallest (level, row of that level) that met one that
 * was not.  Non-zero only without a factorisation. */
int opty_hip_normal_factor_status(opty_hip_normal *h, int32_t *level,
                                  int64_t *row);
/* y = S^-1 r for ncols right-hand sides, column c at r + c*ld / y + c*ld, M(N-1)
 * doubles each in the order of constraints(free), j*(N-1) + i; one column
 * after the other.  Refused before anything is enqueued: null pointers, a bad
 * memory kind, ld < M(N-1), y overlapping r, no successful factorisation. */
int opty_hip_normal_solve(opty_hip_normal *h, const double *r, double *y,
                          int32_t ncols, int64_t ld, int32_t mem);

int opty_hip_device_count(void);
const char *opty_hip_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* OPTY_HIP_H */
