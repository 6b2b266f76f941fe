/*
 * codec_tcc_vol.h -- MED-PEE volume payloads: one bitstream planned across a slice stack
 * (scheme 1).  Same boundary contract as codec_tcc.h (device pointers, a caller-provided
 * workspace, asynchronous on `stream`, no allocation, no host synchronisation, 0 or a negative
 * status with a codec_last_error text).
 *
 * The rule (all integer; specification: tests/pee_volume_spec.py).  caps[B][tmax] are the
 * slices' capacities at T = 1..tmax (codec_pee_capacity), N the stream's bits:
 *   S(T)  = sum over b of caps[b][T-1];  T* = the smallest T with S(T) >= N.  No such T:
 *           status 1, T* = tmax and N is replaced by S(tmax) (the stream's first S(tmax) bits
 *           are embedded, as the per-slice truncation does);
 *   c_b   = caps[b][T*-1], P_b = c_0 + .. + c_(b-1), P_B = S(T*);
 *   even  n_b = floor(N P_(b+1) / P_B) - floor(N P_b / P_B)  (all 0 when P_B = 0): bits in
 *         proportion to capacity, sum n_b = N and n_b <= c_b;
 *   fill  n_b = min(c_b, max(0, N - P_b)): slices filled in order;
 *   T_b   = the smallest T with caps[b][T-1] >= n_b (codec_pee_capacity's rule; <= T*);
 *   off_b = n_0 + .. + n_(b-1): slice b carries stream bits [off_b, off_b + n_b).
 * Streams and payload rows are LSB-first in 64-bit words (bit k of a stream = bit k % 64 of word
 * k / 64); row bits at or above n_b and the gathered stream's pad bits are zero.
 *
 * Bounds every entry checks: B * (H/2) * (W/2) <= 2^31 - 1, 0 <= N <= 2^31 - 1 (so the
 * products N * P stay below 2^62), B * payload_words <= 2^31 - 1.  P->T is ignored; P->maxval
 * and P->bytes are used by the two convenience calls only but checked by all.
 */
#ifndef CODEC_TCC_VOL_H
#define CODEC_TCC_VOL_H

#include "codec_tcc.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CODEC_K_VOL_PLAN 38    /* plan / decode-side offsets: one 1024-thread workgroup   */
#define CODEC_K_VOL_SCATTER 39 /* stream -> payload rows, one thread per row word        */
#define CODEC_K_VOL_GATHER 40  /* payload rows -> stream, one thread per stream word     */

#define CODEC_VOL_EVEN 0
#define CODEC_VOL_FILL 1

typedef struct codec_pee_volume_info {
    int32_t status;    /* 0, or 1: no T <= tmax holds the stream (truncated to `total`)    */
    int32_t T;         /* T*                                                              */
    int32_t total;     /* bits planned: min(N, S(tmax)) = off[B]                          */
    int32_t requested; /* N                                                               */
    int32_t capacity;  /* S(T*)                                                           */
    int32_t policy, B, tmax;
} codec_pee_volume_info;

/* Bytes of the volume workspace for P's shape and row pitch and this tmax (1..64): the plan's
 * capacity curves, the payload rows [B][payload_words] and the decode side's offsets.  The
 * decode-side calls (gather, extract) need the size for tmax = 1.  0 for bad arguments.  The
 * calls keep no state in it. */
size_t codec_pee_volume_workspace_bytes(const codec_pee_params* P, int32_t tmax);

/* caps [B][tmax] (device int32; a value is taken as min(max(value, 0), (H/2)(W/2))), nbits = N,
 * policy -> n_out[B], t_out[B], off_out[B + 1] (device int32) and one info record.  Requires
 * 64 * P->payload_words >= min(N, (H/2)(W/2)), so that every n_b fits a payload row.  One
 * launch of one workgroup. */
int codec_pee_volume_plan(const codec_pee_params* P, const int32_t* caps, int32_t tmax, int64_t nbits,
                          int32_t policy, int32_t* n_out, int32_t* t_out, int32_t* off_out,
                          codec_pee_volume_info* info, void* stream);

/* rows[B][payload_words]: row b = stream bits [off[b], off[b] + n[b]), zero above (every row
 * word is written).  bitstream holds ceil(nbits / 64) words and is never read past them;
 * n[b] is taken as min(max(n[b], 0), 64 * payload_words) and off[b] as max(off[b], 0). */
int codec_pee_volume_scatter(const codec_pee_params* P, const uint64_t* bitstream, int64_t nbits,
                             const int32_t* n, const int32_t* off, uint64_t* rows, void* stream);

/* The inverse: the records' L (device; a negative L counts as 0, and L is capped at
 * min(64 * payload_words, (H/2)(W/2))) are scanned into offsets, and the first L_b bits of row b
 * are concatenated into bitstream[stream_words]; every word is written exactly once, words and
 * bits past the embedded total as zero (a stream shorter than the total is cut).  total_out
 * (device int32) = the embedded total.  Two launches. */
int codec_pee_volume_gather(const codec_pee_params* P, const codec_pee_meta* meta, const uint64_t* rows,
                            uint64_t* bitstream, int64_t stream_words, int32_t* total_out, void* workspace,
                            size_t workspace_bytes, void* stream);

/* codec_pee_capacity -> plan -> scatter -> codec_pee_embed_ts on one stream, with results
 * identical to the separate calls.  stego == cover is allowed (the capacity pass reads the
 * cover before the embed writes it).  pee_workspace: codec_pee_workspace_bytes(P), with its
 * rules; vol_workspace: codec_pee_volume_workspace_bytes(P, tmax). */
int codec_pee_volume_embed(const codec_pee_params* P, const void* cover, void* stego, const uint64_t* bitstream,
                           int64_t nbits, int32_t policy, int32_t tmax, int32_t* n_out, int32_t* t_out,
                           int32_t* off_out, codec_pee_volume_info* info, codec_pee_meta* meta, uint64_t* lm,
                           void* pee_workspace, size_t pee_workspace_bytes, void* vol_workspace,
                           size_t vol_workspace_bytes, void* stream);

/* codec_pee_extract -> gather on one stream (the record contract of codec_pee_extract holds). */
int codec_pee_volume_extract(const codec_pee_params* P, const void* stego, const codec_pee_meta* meta,
                             const uint64_t* lm, void* cover_out, uint64_t* bitstream, int64_t stream_words,
                             int32_t* total_out, void* pee_workspace, size_t pee_workspace_bytes,
                             void* vol_workspace, size_t vol_workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CODEC_TCC_VOL_H */
