// codec_vol_checks.h -- what the volume family's entries (codec_vol.hip, codec_gvol.hip) check
// alike, and the head their workspaces share.  The texts carry the entry's name (`who`).
#pragma once
#include <algorithm>

#include "codec_common.h"
#include "codec_tcc_gate.h"
#include "codec_tcc_vol.h"

static inline long long vol_nc(const codec_pee_params* P) { return (long long)(P->H / 2) * (P->W / 2); }

// the checks every entry shares: codec_pee's own and the volume bounds; max_nc: the gated
// entries' bound on a slice's candidates, CODEC_PEE_GATE_MAX_NC (0: none)
static inline int vol_check(const codec_pee_params* P, const char* who, long long max_nc = 0) {
    if (!P) return set_err(CODEC_EINVAL, "%s: params is NULL", who);
    if (P->B < 1 || P->H < 1 || P->W < 1 || (long long)P->H * P->W > 0x7FFFFFFFLL)
        return set_err(CODEC_EINVAL, "%s: bad shape B=%d H=%d W=%d", who, P->B, P->H, P->W);
    if (P->bytes != 1 && P->bytes != 2) return set_err(CODEC_EINVAL, "%s: bytes must be 1 or 2", who);
    if (P->T < 1) return set_err(CODEC_EINVAL, "%s: T must be >= 1", who);
    const int vmax = P->bytes == 2 ? 65535 : 255;
    if (P->maxval < 1 || P->maxval > vmax) return set_err(CODEC_EINVAL, "%s: maxval out of range", who);
    if (P->payload_words < 1 || P->lm_words < 1)
        return set_err(CODEC_EINVAL, "%s: payload_words/lm_words must be >= 1", who);
    const long long nc = vol_nc(P);
    if ((long long)P->lm_words * 64 < nc) return set_err(CODEC_EINVAL, "%s: lm_words must cover every candidate", who);
    if (max_nc && nc > max_nc) return set_err(CODEC_EINVAL, "%s: more than 2^26 candidates per slice", who);
    if ((long long)P->B * nc > 0x7FFFFFFFLL)
        return set_err(CODEC_EINVAL, "%s: B * (H/2) * (W/2) = %lld exceeds 2^31 - 1", who, (long long)P->B * nc);
    if ((long long)P->B * P->payload_words > 0x7FFFFFFFLL)
        return set_err(CODEC_EINVAL, "%s: B * payload_words exceeds 2^31 - 1", who);
    return 0;
}

static inline int vol_check_tmax(int32_t tmax, int tmax_max, const char* who) {
    if (tmax < 1 || tmax > tmax_max) return set_err(CODEC_EINVAL, "%s: tmax must be in 1..%d", who, tmax_max);
    return 0;
}

// the plan's arguments, in the order their errors are reported; g_fixed: the gated entries'
// (the ungated ones pass -1, which holds)
static inline int vol_check_plan(const codec_pee_params* P, int32_t tmax, int tmax_max, int64_t nbits, int32_t policy,
                                 int32_t g_fixed, const char* who) {
    int rc = vol_check_tmax(tmax, tmax_max, who);
    if (rc) return rc;
    if (nbits < 0 || nbits > 0x7FFFFFFFLL) return set_err(CODEC_EINVAL, "%s: nbits must be in 0..2^31 - 1", who);
    if (policy != CODEC_VOL_EVEN && policy != CODEC_VOL_FILL)
        return set_err(CODEC_EINVAL, "%s: policy must be CODEC_VOL_EVEN or CODEC_VOL_FILL", who);
    if (g_fixed < -1 || g_fixed > CODEC_PEE_GATE_MAX)
        return set_err(CODEC_EINVAL, "%s: g_fixed must be -1 or in 0..65535", who);
    if (64ll * P->payload_words < std::min<long long>(nbits, vol_nc(P)))
        return set_err(CODEC_EINVAL, "%s: payload_words = %d cannot hold a slice's share of %lld bits", who,
                       P->payload_words, (long long)nbits);
    return 0;
}

static inline int vol_check_stream_words(int64_t stream_words, const char* who) {
    // one thread per word in blocks of 256; a stream never holds more than 2^31 - 1 bits
    if (stream_words < 0 || stream_words > (1ll << 25))
        return set_err(CODEC_EINVAL, "%s: stream_words must be in 0..2^25", who);
    return 0;
}

static inline int vol_check_pee_ws(const codec_pee_params* P, size_t pee_workspace_bytes, const char* who) {
    const size_t need_pee = codec_pee_workspace_bytes(P);
    if (!need_pee || pee_workspace_bytes < need_pee)
        return set_err(CODEC_EINVAL, "%s: PEE workspace too small (%zu < %zu)", who, pee_workspace_bytes, need_pee);
    return 0;
}

// the head of every volume workspace: the B + 1 offsets, then the payload rows; `end`: where the
// unit's own tables begin.  codec_pee_volume_gather reads the head alone, so it takes a gated
// volume workspace as it is.
struct VolWsHead {
    size_t off, rows, end;
};
static inline VolWsHead vol_ws_head(const codec_pee_params* P) {
    VolWsHead L;
    L.off = 0;
    L.rows = align_up(((size_t)P->B + 1) * 4, 256);
    L.end = align_up(L.rows + (size_t)P->B * P->payload_words * 8, 256);
    return L;
}
