/*
 * pasco_grad.h -- flat C ABI of the training kernels of the sparse convolution family in libpascohip.so
 * (pasco_amd/csrc/grad.hip).
 *
 * A sparse convolution is out[o] = sum_k [nbr[k][o] >= 0] in[nbr[k][o]] @ W[k] + bias over a neighbour table nbr int32
 * [K, n_out] (-1 = no neighbour).  Its three gradients for an upstream gradient dy [n_out, cout] are
 *
 *   d_in[i]  = sum_k [inv[k][i] >= 0] dy[inv[k][i]] @ W[k]^T      the SAME operation over the inverted table: it runs on
 *                                                                 ph_conv_fwd (include/pasco_hip.h), pg_nbr_invert builds inv
 *   d_W[k]   = sum_o [nbr[k][o] >= 0] in[nbr[k][o]]^T dy[o]       pg_conv_wgrad
 *   d_bias   = sum_o dy[o]                                        pg_colsum
 *
 * The host restatement is pasco_amd/grad/host.py.  A separate surface from include/pasco_hip.h: own prefix, own version, no
 * CPU oracle.
 *
 * Conventions (as pasco_waffle.h): device pointers only; all work is enqueued on `stream`; no call synchronises, allocates or
 * reads the host or the environment; return 0 = ok, text of a failure via pg_last_error().  Matrices are row-major fp32.
 *
 * Determinism: no floating-point atomics anywhere.  Every sum has one fixed order that depends on the shapes alone (never on
 * the number of compute units or on timing), so a call repeated on the same inputs returns the same bits.
 */
#ifndef PASCO_GRAD_H_
#define PASCO_GRAD_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PG_FN(name) pg_##name

#define PG_ABI_VERSION 1
#define PG_MAX_KVOL 64                       /* kernel offsets of one table */
#define PG_SLAB_ROWS 256                     /* pg_conv_wgrad: output rows per slab before the workspace cap applies */
#define PG_WGRAD_WORKSPACE_CAP (64ll << 20)  /* pg_conv_wgrad: its workspace never exceeds this many bytes */
#define PG_COLSUM_ROWS 1024                  /* pg_colsum: rows per partial sum */

int PG_FN(abi_version)(void);
const char *PG_FN(last_error)(void);

/* nbr int32 [K, n_out] with values in [-1, n_in) -> inv int32 [K, n_in]: inv[k][nbr[k][o]] = o, -1 everywhere else.
 * PRECONDITION: for a fixed k, the o with nbr[k][o] >= 0 have distinct nbr[k][o] (o -> input row is injective per offset), so
 * the plain stores do not race.  It holds for every map the library serves: stride-1 odd kernels (a translation), kernel ==
 * stride down-convolutions (every input has one parent) and the kernel 2 / stride 2 generative transpose (every child has one
 * parent).  A table that breaks it gives, per (k, i), one of the candidate rows.  Values outside [-1, n_in) are skipped.
 * One fill and one scatter launch; n_out == 0 fills only; n_in == 0 is a no-op.  1 <= K <= PG_MAX_KVOL. */
int PG_FN(nbr_invert)(const int32_t *nbr, int32_t K, int64_t n_out, int64_t n_in, int32_t *inv, void *stream);

/* Output rows per slab pg_conv_wgrad uses at this shape: PG_SLAB_ROWS, doubled until the slabs' partial results
 * (slabs * K * cin * cout * 4 bytes) fit into PG_WGRAD_WORKSPACE_CAP or one slab holds every row.  A function of the four
 * numbers alone.  -1 for a shape outside the served range. */
int64_t PG_FN(wgrad_slab_rows)(int32_t K, int32_t cin, int32_t cout, int64_t n_out);

/* Bytes of workspace pg_conv_wgrad needs at this shape (0 when one slab holds every row: it then writes dw itself). */
int64_t PG_FN(wgrad_workspace_bytes)(int32_t K, int32_t cin, int32_t cout, int64_t n_out);

/* x fp32 [n_in, cin], dy fp32 [n_out, cout], nbr int32 [K, n_out] -> dw fp32 [K, cin, cout] (overwritten, not accumulated):
 *   dw[k] = sum over the o with 0 <= nbr[k][o] < n_in of x[nbr[k][o]]^T dy[o]
 * Exact fp32 products and sums (v_mfma_f32_32x32x2_f32; the rows are the contraction).  A workgroup owns one offset, one slab
 * of consecutive output rows and one (cin tile, cout tile); it adds the slab's rows in ascending order and writes its partial
 * tile; a second launch adds the slabs' partials in ascending slab order.  Any 1 <= cin, cout; 1 <= K <= PG_MAX_KVOL;
 * n_out == 0 writes zeros.  `workspace` holds at least pg_wgrad_workspace_bytes() bytes, 4-byte aligned (unused when that is 0). */
int PG_FN(conv_wgrad)(const float *x, int64_t n_in, int32_t cin, const float *dy, int64_t n_out, int32_t cout,
                      const int32_t *nbr, int32_t K, float *dw, void *workspace, int64_t workspace_bytes, void *stream);

/* Bytes of workspace pg_colsum needs (0 when n <= PG_COLSUM_ROWS). */
int64_t PG_FN(colsum_workspace_bytes)(int64_t n, int32_t c);

/* dy fp32 [n, c] -> out fp32 [c] = sum over the rows (overwritten).  Partial sums over PG_COLSUM_ROWS consecutive rows (four
 * interleaved chains of every fourth row, added 0 + 1 + 2 + 3), then the partials in ascending order.  n == 0 writes zeros. */
int PG_FN(colsum)(const float *dy, int64_t n, int32_t c, float *out, void *workspace, int64_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* PASCO_GRAD_H_ */
