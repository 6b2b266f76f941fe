/*
 * codec_tcc_gvol.h -- gated MED-PEE volume payloads (scheme 1): one bitstream planned across a
 * slice stack over (T, G), the meeting of codec_tcc_vol.h (the stream, its shares, the payload
 * rows) and codec_tcc_gate.h (the smoothness gate, its capacity table, the selection rule).
 * Same boundary contract as codec_tcc.h (device pointers, caller-provided workspaces,
 * asynchronous on `stream`, no allocation, no host synchronisation, capturable into a graph,
 * 0 or a negative status with a codec_last_error text).
 *
 * The rule (all integer; specification: tests/pee_gvol_spec.py).  Per slice b the gated table
 * n_b[16], hs_b[tmax][16] with K_b(T, j), N_b(j), A_b(T, j) as codec_tcc_gate.h defines them; N
 * the stream's bits; a policy.
 *   1. volume choice   n[j] = sum_b n_b[j], hs[u][j] = sum_b hs_b[u][j]; (T*, j*) = the gate
 *      header's selection rule on the summed table with L = N (K >= N and K > 0, the smallest
 *      A / K, ties to the smaller T, then the smaller j; N = 0 gives (1, 0)).  The summed A
 *      reaches 2^41 and K 2^31: A1 K2 < A2 K1 is compared exactly as 128-bit products.  No
 *      feasible pair: status 1, (T*, j*) = (tmax, 15) and N is replaced by K(tmax, 15) -- the
 *      stream's first bits are embedded, the ungated volume's truncation.  G* = GATES[j*].
 *   2. shares          c_b = K_b(T*, j*), P_b = c_0 + .. + c_(b-1), P_B their sum; n_b and
 *      off_b by codec_tcc_vol.h's even / fill formulas on these c_b: sum n_b = N, n_b <= c_b.
 *   3. per slice       (T_b, j_b) = the selection rule on slice b's own table with L = n_b,
 *      G_b = GATES[j_b].  (T*, j*) is feasible for slice b (K_b(T*, j*) = c_b >= n_b), so the
 *      rule finds a pair with K_b(T_b, j_b) >= n_b: no slice is truncated, every record has
 *      status 0 and the volume's status lives in the info record.  n_b = 0 gives (1, 0).
 *   fixed gate g (g_fixed >= 0): the tables are the two-class ones of that gate (column 0 =
 *      D <= g), and the rule is codec_tcc_vol.h's on caps[b][T-1] = K_b(T, 0): T* = the
 *      smallest T whose summed K(T, 0) holds N (none: status 1, T* = tmax, N := K(tmax, 0)),
 *      T_b = the smallest T with K_b(T, 0) >= n_b, G_b = g.
 * The records are ordinary gated scheme-1 records (reserved[1] = G_b + 1): every slice decodes
 * on its own through codec_pee_gate_extract.
 *
 * Bounds every entry checks before any device operation: those of codec_tcc_vol.h
 * (B * (H/2) * (W/2) <= 2^31 - 1, 0 <= N <= 2^31 - 1, B * payload_words <= 2^31 - 1) and of
 * codec_tcc_gate.h (tmax <= 16, (H/2) * (W/2) <= 2^26).  A table value is taken as
 * min(value, (H/2)(W/2)) and a slice's c_b as min(K_b(T*, j*), (H/2)(W/2)), so that the shares
 * fit their payload rows and N * P stays below 2^62 whatever the buffers hold.
 */
#ifndef CODEC_TCC_GVOL_H
#define CODEC_TCC_GVOL_H

#include "codec_tcc_gate.h"
#include "codec_tcc_vol.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CODEC_K_GVOL_PLAN 42 /* the (T, G) volume plan: one 1024-thread workgroup, one launch */

typedef struct codec_pee_gvol_info {
    int32_t status;    /* 0, or 1: no (T, G) holds the stream (truncated to `total`)       */
    int32_t T;         /* T*                                                              */
    int32_t total;     /* bits planned = off[B]                                           */
    int32_t requested; /* N                                                               */
    int32_t capacity;  /* the stack's capacity at (T*, G*) = the sum of c_b               */
    int32_t policy, B, tmax;
    int32_t gate;      /* the gate VALUE G* (g_fixed for a fixed gate)                    */
    int32_t reserved;  /* 0                                                               */
} codec_pee_gvol_info;

/* Bytes of the gated volume workspace for P's shape and row pitch and this tmax (1..16): the
 * decode side's offsets, the payload rows [B][payload_words] and the slices' tables.  Its head
 * is a codec_pee_volume_workspace_bytes(P, 1) workspace.  The decode side needs the size for
 * tmax = 1.  0 for bad arguments.  The calls keep no state in it. */
size_t codec_pee_gvol_workspace_bytes(const codec_pee_params* P, int32_t tmax);

/* n [B][16] and hs [B][tmax][16] (device uint32, as codec_pee_gate_capacity writes them; with
 * g_fixed >= 0 the two-class tables of that gate), nbits = N, policy (CODEC_VOL_EVEN / _FILL),
 * g_fixed (-1 for the ladder, or 0..65535) -> n_out[B], t_out[B], g_out[B] (gate VALUES),
 * off_out[B + 1] (device int32) and one info record.  Requires 64 * P->payload_words >=
 * min(N, (H/2)(W/2)).  One launch of one workgroup. */
int codec_pee_gvol_plan(const codec_pee_params* P, const uint32_t* n, const uint32_t* hs, int32_t tmax, int64_t nbits,
                        int32_t policy, int32_t g_fixed, int32_t* n_out, int32_t* t_out, int32_t* g_out,
                        int32_t* off_out, codec_pee_gvol_info* info, void* stream);

/* codec_pee_gate_capacity (the table alone) -> plan -> codec_pee_volume_scatter ->
 * codec_pee_gate_embed on one stream, with results identical to the separate calls.
 * stego == cover is allowed (the table pass reads the cover before the embed writes it).
 * pee_workspace: codec_pee_workspace_bytes(P), with its rules; table_workspace:
 * codec_pee_gate_workspace_bytes(P, tmax) -- only its tail, the table's bins, is used, so it
 * needs no reset and may be pee_workspace itself when that is large enough; gvol_workspace:
 * codec_pee_gvol_workspace_bytes(P, tmax). */
int codec_pee_gvol_embed(const codec_pee_params* P, const void* cover, void* stego, const uint64_t* bitstream,
                         int64_t nbits, int32_t policy, int32_t tmax, int32_t g_fixed, int32_t* n_out, int32_t* t_out,
                         int32_t* g_out, int32_t* off_out, codec_pee_gvol_info* info, codec_pee_meta* meta,
                         uint64_t* lm, void* pee_workspace, size_t pee_workspace_bytes, void* table_workspace,
                         size_t table_workspace_bytes, void* gvol_workspace, size_t gvol_workspace_bytes, void* stream);

/* codec_pee_gate_extract -> codec_pee_volume_gather on one stream (the record contract of
 * codec_pee_extract holds; ungated records decode too).  gvol_workspace:
 * codec_pee_gvol_workspace_bytes(P, 1) or more. */
int codec_pee_gvol_extract(const codec_pee_params* P, const void* stego, const codec_pee_meta* meta, const uint64_t* lm,
                           void* cover_out, uint64_t* bitstream, int64_t stream_words, int32_t* total_out,
                           void* pee_workspace, size_t pee_workspace_bytes, void* gvol_workspace,
                           size_t gvol_workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CODEC_TCC_GVOL_H */
