/*
 * pasco_attngrad.h -- flat C ABI of the backward of the masked cross-attention in libpascohip.so
 * (pasco_amd/csrc/attn_grad.hip).
 *
 * The forward is ph_attn_cross_fwd of include/pasco_hip.h: per subnet b and head h, out = softmax(q k^T + mask) v with a
 * few queries (<= 128) over very many keys, streamed with an online softmax; the [B*H, Qn, N] score tensor never exists.  The
 * backward here has the same property.  With P = softmax(q k^T + mask) and delta[q] = sum_d dout[q][d] * out[q][d]:
 *
 *   dV[key] = sum_q P[q][key] dout[q]
 *   dP[q][key] = dout[q] . v[key]
 *   dS = P * (dP - delta[q])
 *   dK[key] = sum_q dS[q][key] q[q]
 *   dQ[q]   = sum_key dS[q][key] k[key]
 *
 * dq is the gradient with respect to the PRE-SCALED q that was passed in (the 1/sqrt(Dh) is the caller's multiplication).  The
 * mask carries no gradient.  The host restatement is pasco_amd/grad/host.py (attn_cross_bwd).  A separate surface from
 * include/pasco_hip.h: own prefix, own version, no CPU oracle.
 *
 * Layouts (the forward's):  q, dq [B, H, Qn, Dh];  k, v, dk, dv [B, N, H*Dh];  out, dout [B, Qn, H*Dh];
 *   bits uint32 [B, N, 4]: bit q of a key's 128-bit word = query q may attend to the key, or NULL = no mask;
 *   any  uint32 [B, 4]: OR over the keys of bits, or NULL.
 * Mask rules (the forward's): bits at positions >= Qn are never looked at; a query with no allowed key attends everywhere when
 * `any` is given; with bits given and any == NULL such a query has a zero output row, contributes nothing to any gradient, and
 * its dq row is exact zeros.
 *
 * Conventions (as pasco_grad.h): device pointers only; all work is enqueued on `stream`; no call synchronises, allocates or
 * reads the host or the environment; return 0 = ok, text of a failure via pa_last_error().  A refused call launches nothing.
 * Served: dh == 48, 1 <= qn <= 128, b, h, n >= 1, finite inputs.
 *
 * Determinism: no floating-point atomics anywhere.  Every key belongs to one key range, whose owner writes its dK / dV rows
 * with plain stores; dQ is summed over the ranges in ascending order; the number of ranges is a function of (n, b, h) alone.
 * A call repeated on the same inputs returns the same bits.
 */
#ifndef PASCO_ATTNGRAD_H_
#define PASCO_ATTNGRAD_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PA_FN(name) pa_##name

#define PA_ABI_VERSION 1
#define PA_DH 48                             /* the head dimension served */
#define PA_MAX_Q 128                         /* queries served */

int PA_FN(abi_version)(void);
const char *PA_FN(last_error)(void);

/* Bytes of scratch the two calls below need for a shape: the row statistics, the per-range partial (m, l) of the statistics
 * pass and the per-range partial dQ.  0 for a shape that is not served. */
int64_t PA_FN(attn_bwd_workspace_bytes)(int64_t n, int32_t b, int32_t h, int32_t qn, int32_t dh);

/* The statistics pass alone: lse[b, h, q] = log sum_key exp(s[q][key]) over the allowed keys (+inf for a query with nothing
 * allowed: every P of that row is then 0) and delta[b, h, q] = sum_d dout[q][d] * out[q][d], both fp32 [B, H, Qn], overwritten.
 * pa_attn_cross_bwd runs this pass itself; the entry exists for timing and for tests. */
int PA_FN(attn_bwd_stats)(const float *q, const float *k, const uint32_t *bits, const uint32_t *any, const float *out,
                          const float *dout, float *lse, float *delta, int64_t n, int32_t b, int32_t h, int32_t qn,
                          int32_t dh, void *ws, int64_t ws_bytes, void *stream);

/* dq, dk, dv (each overwritten; any of them may be NULL = not wanted, not all three) from the forward's operands, its result
 * `out` and the incoming gradient `dout`.  A NULL output changes no bit of the other two. */
int PA_FN(attn_cross_bwd)(const float *q, const float *k, const float *v, const uint32_t *bits, const uint32_t *any,
                          const float *out, const float *dout, float *dq, float *dk, float *dv, int64_t n, int32_t b,
                          int32_t h, int32_t qn, int32_t dh, void *ws, int64_t ws_bytes, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* PASCO_ATTNGRAD_H_ */
