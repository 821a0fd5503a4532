/*
 * pasco_optim.h -- flat C ABI of the optimiser step in libpascohip.so (pasco_amd/csrc/optim.hip): AdamW with decoupled weight
 * decay over any number of fp32 tensors, the global L2 norm of their gradients and the clip by it folded into the update.  The
 * optimiser class over it is pasco_amd/grad/optim.py (`AdamW`), the host restatement pasco_amd/grad/host.py (`optim_*`).  A
 * separate surface from include/pasco_hip.h: own prefix, own version, no CPU oracle.
 *
 * Conventions (as pasco_norm.h): device pointers only; all work is enqueued on `stream`; no call synchronises, allocates or
 * reads the host or the environment; return 0 = ok, text of a failure via po_last_error().  No floating-point atomics, no
 * in-launch ticket or fence: the three launches of a step are ordered by the stream, and the same inputs give the same bits on
 * every run.
 *
 * Tables (device memory; the caller uploads them once and again only when a pointer or the set of tensors changes):
 *   tensors[T]  po_tensor: the parameter p, its gradient g, the two moments m and v (fp32, n elements each, contiguous),
 *               the index of its hyper-parameter group and the index of its state record.  Two entries never share a state
 *               record or memory.
 *   chunks[C]   po_chunk: (tensor, start).  A chunk is the elements [start, min(start + PO_CHUNK, n)) of one tensor, start a
 *               multiple of PO_CHUNK; the chunks of a table cover every element of every tensor once.  A tensor of 0 elements
 *               has no chunk.
 * One launch covers the whole table: any number of tensors of any size, 0 <= T < 2^31, n < 2^31 per tensor, less than 2^40
 * elements in total (po_table_check states these limits for the caller that builds the tables on the host).
 *
 * Element access: inside a chunk thread t of 256 owns the quads q = t, t + 256, ... (elements 4 q .. 4 q + 3 of the chunk).
 * A whole quad is moved by one 16-byte access where p, g, m and v of the tensor are all 16-byte aligned (the chunk start is
 * a multiple of 4), by 4-byte accesses otherwise and at the ragged end of a tensor.  Which access is used changes no result.
 *
 * State (device memory, one po_state per tensor that ever had a gradient): step, beta1^step, beta2^step - per tensor, as in
 * torch: a tensor that first receives a gradient late gets the bias correction of step 1.  A fresh record is (0, 1.0, 1.0).
 *
 * The step, with s the clip scale of po_prepare and per-tensor fp32 scalars formed in fp64 and rounded once
 *   decay = 1 - lr * wd,  omb1 = 1 - beta1,  b2 = beta2,  omb2 = 1 - beta2,  bc2sqrt = sqrt(1 - beta2^step),  eps,
 *   neg_step = -lr / (1 - beta1^step)
 * is per element, in fp32, every operation rounded on its own (no contraction), in this order:
 *   g' = g * s;  p = p * decay;  m = m + (g' - m) * omb1;  v = v * b2 + (g' * g') * omb2;
 *   d = sqrt(v) / bc2sqrt + eps;  p = p + (m / d) * neg_step
 * - the operations of torch's single-tensor AdamW with the clip folded in, so the gradients are read twice and never written.
 */
#ifndef PASCO_OPTIM_H_
#define PASCO_OPTIM_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PO_FN(name) po_##name

#define PO_ABI_VERSION 1
#define PO_CHUNK 4096                        /* elements of one chunk (a multiple of 1024) */
#define PO_MAX_GROUPS 8                      /* hyper-parameter groups of one step */
#define PO_POLICY_PROPAGATE 0                /* a non-finite gradient makes the weights non-finite, as in torch */
#define PO_POLICY_SKIP 1                     /* a non-finite gradient skips the step: nothing moves, the skipped count does */

typedef struct {
  float *p;                /* the parameter, updated in place */
  const float *g;          /* its gradient, read only */
  float *m, *v;            /* exp_avg, exp_avg_sq, updated in place */
  int64_t n;               /* elements */
  int32_t group;           /* 0 .. n_groups - 1 */
  int32_t state;           /* index into states[] and scalars[] */
} po_tensor;               /* 48 bytes */

typedef struct {
  int32_t tensor;          /* index into tensors[] */
  int32_t start;           /* first element, a multiple of PO_CHUNK */
} po_chunk;                /* 8 bytes */

typedef struct {
  int64_t step;
  double beta1_pow, beta2_pow;       /* beta1^step, beta2^step */
} po_state;                /* 24 bytes */

typedef struct {
  double sumsq;            /* sum of g * g over every element of the table, exact products, fp64 sum */
  double norm;             /* grad_scale * sqrt(sumsq) */
  int64_t skipped;         /* steps skipped so far under PO_POLICY_SKIP; po_prepare adds to it, the caller zeroes it once */
} po_result;               /* 24 bytes */

typedef struct {
  float clip;              /* s: what every gradient element is multiplied by */
  int32_t apply;           /* 0: po_adamw returns at once */
} po_step;                 /* 8 bytes */

typedef struct {
  float decay, omb1, b2, omb2, bc2sqrt, eps, neg_step, unused;
} po_scalars;              /* 32 bytes, one per state record */

typedef struct {
  double lr, beta1, beta2, eps, weight_decay;
} po_group;

typedef struct {
  po_group g[PO_MAX_GROUPS];
} po_groups;               /* passed by value */

int PO_FN(abi_version)(void);
const char *PO_FN(last_error)(void);

/* The limits of a table, for the host that builds one: T tensors, the largest has max_n elements, `total` elements in all,
 * n_groups groups.  0 = served; otherwise the text says which limit. */
int PO_FN(table_check)(int64_t T, int64_t max_n, int64_t total, int32_t n_groups);

/* Launch 1.  partials fp64 [C]: per chunk the sum of (double)g * (double)g over its elements (the products are exact; a
 * thread adds its elements in ascending order, the 256 threads are combined in a fixed tree). */
int PO_FN(sqnorm)(const po_tensor *tensors, int32_t T, const po_chunk *chunks, int64_t C, double *partials, void *stream);

/* Launch 2 (one workgroup).  Adds the C partials in an order that depends on C alone and writes result->sumsq and
 * result->norm.  The clip scale, in fp64: c = max_norm > 0 ? min(max_norm / (norm + 1e-6), 1) : 1 (a NaN stays a NaN, as in
 * torch's clamp);  step->clip = (float)(c * grad_scale).
 * If sumsq is finite, or policy is PO_POLICY_PROPAGATE: step->apply = 1 and for each of the T tensors its state record
 * advances (step += 1, both powers multiplied by the group's beta in fp64) and scalars[state] is written from the advanced
 * record.  Otherwise (PO_POLICY_SKIP and a non-finite sumsq - which happens exactly when some gradient element is inf or NaN,
 * since fp32 squares cannot overflow an fp64 sum): step->apply = 0, result->skipped += 1, no state record is touched. */
int PO_FN(prepare)(const po_tensor *tensors, int32_t T, const double *partials, int64_t C, po_groups groups, int32_t n_groups,
                   double max_norm, double grad_scale, int32_t policy, po_state *states, po_scalars *scalars,
                   po_result *result, po_step *step, void *stream);

/* Launch 3.  The update above over every chunk: reads p, g, m, v, writes p, m, v (28 bytes per element).  The grid is capped
 * and strides over the chunks. */
int PO_FN(adamw)(const po_tensor *tensors, int32_t T, const po_chunk *chunks, int64_t C, const po_scalars *scalars,
                 const po_step *step, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* PASCO_OPTIM_H_ */
