// record.hip — the sample record of the C ABI (include/isingmc_hip.h, isingmc_record_*): p = 0 states kept on the device, read back as
// rows, or reduced there to bit series and autocorrelations (observe.hip, sse_observe.hip.h).
#include "batch.hip.h"
#include "sse_launch.h"

#include <algorithm>
#include <cstdio>

using namespace sse;

// Append the p = 0 states to the sample record: a device-to-device copy of dev.state (current in HBM after every launch) on the
// batch's stream, behind the last launch of a sampled step.  The caller has checked the room (isingmc_timesteps).
hipError_t sse::record_append(isingmc_batch *b) {
    const size_t row = (size_t)b->dev.R * b->dev.nwords;
    if (b->rec_count >= b->rec_cap) return hipErrorInvalidValue;
    const hipError_t e = hipMemcpyAsync(b->rec.as<uint32_t>() + (size_t)b->rec_count * row, b->dev.state, row * sizeof(uint32_t), hipMemcpyDeviceToDevice, b->stream);
    if (e == hipSuccess) b->rec_count++;
    return e;
}

static int rec_fail_alloc(isingmc_batch *b, const char *what, size_t bytes) {
    (void)hipGetLastError();
    char buf[160];
    snprintf(buf, sizeof buf, "sample record: hipMalloc of %zu bytes (%s) failed", bytes, what);
    b->err = buf;
    return ISINGMC_ENODEVICE;
}
// a scratch buffer of at least `bytes`, kept for the next call
static int rec_grow(isingmc_batch *b, DevBuf &buf, size_t bytes, const char *what) {
    return buf.reserve(bytes, b->stream) == hipSuccess ? ISINGMC_OK : rec_fail_alloc(b, what, bytes);
}
static int rec_range(isingmc_batch *b, uint32_t first, uint32_t count) {
    if (!b->rec) { b->err = "no sample record attached (isingmc_record_attach)"; return ISINGMC_EINVAL; }
    if (count == 0 || first > b->rec_count || count > b->rec_count - first) { b->err = "sample record: bad row range"; return ISINGMC_EINVAL; }
    return ISINGMC_OK;
}

// checks the groups, uploads them and runs record_series_kernel into the batch's series buffer: [R][ngroups][(count + 31) / 32]
static int rec_make_series(isingmc_batch *b, uint32_t ngroups, const uint32_t *group_start, const uint32_t *group_vars, const uint8_t *group_flip,
                           uint32_t first, uint32_t count) {
    if (!ngroups || !group_start || !group_vars) { b->err = "sample record: no observable groups"; return ISINGMC_EINVAL; }
    if (const int rc = rec_range(b, first, count)) return rc;
    if (const int rc = check_groups(b, "sample record", ngroups, group_start, group_vars, b->dev.N)) return rc;
    const uint32_t nv = group_start[ngroups];
    if (4 * obs_series_lds_words(b->dev.nwords) > 4 * b->lds_total_words) {
        b->err = "sample record: 64 state rows of this model exceed LDS (record_series_kernel stages them there)";
        return ISINGMC_ENOTIMPL;
    }
    HIP_TRY(b, hipSetDevice(b->device));
    // groups: [ngroups + 1] starts, [nv] variables, [ngroups] flip bytes
    const size_t o_vars = (size_t)(ngroups + 1) * 4, o_flip = o_vars + (size_t)nv * 4;
    if (const int rc = rec_grow(b, b->obs_groups, o_flip + ngroups, "observable groups")) return rc;
    const size_t Tw = (count + 31u) / 32u;
    if (const int rc = rec_grow(b, b->obs_series, (size_t)b->dev.R * ngroups * Tw * 4, "bit series")) return rc;
    char *gbuf = b->obs_groups.as<char>();
    HIP_TRY(b, hipMemcpyAsync(gbuf, group_start, o_vars, hipMemcpyHostToDevice, b->stream));
    HIP_TRY(b, hipMemcpyAsync(gbuf + o_vars, group_vars, (size_t)nv * 4, hipMemcpyHostToDevice, b->stream));
    if (group_flip) HIP_TRY(b, hipMemcpyAsync(gbuf + o_flip, group_flip, ngroups, hipMemcpyHostToDevice, b->stream));
    ObsGroups G{ngroups, (const uint32_t *)gbuf, (const uint32_t *)(gbuf + o_vars), group_flip ? (const uint8_t *)(gbuf + o_flip) : nullptr};
    const uint32_t *rows = b->rec.as<uint32_t>() + (size_t)first * b->dev.R * b->dev.nwords;
    const hipError_t e = launch_record_series(b->stream, rows, b->dev.R, b->dev.nwords, count, G, b->obs_series.as<uint32_t>());
    if (e != hipSuccess) { b->err = std::string("record_series launch: ") + hipGetErrorString(e); return ISINGMC_ENODEVICE; }
    return ISINGMC_OK;
}

extern "C" {

int isingmc_record_attach(isingmc_batch *b, uint32_t capacity) {
    if (!b) return ISINGMC_EINVAL;
    if (capacity > (1u << 20)) { b->err = "sample record: capacity above 2^20 samples"; return ISINGMC_EINVAL; }
    HIP_TRY(b, hipSetDevice(b->device));
    if (b->rec) { HIP_TRY(b, hipStreamSynchronize(b->stream)); b->rec.reset(); }
    b->rec_cap = b->rec_count = 0;
    if (capacity == 0) return ISINGMC_OK;
    const size_t bytes = (size_t)capacity * b->dev.R * b->dev.nwords * sizeof(uint32_t);
    if (b->rec.alloc(bytes) != hipSuccess) return rec_fail_alloc(b, "record", bytes);
    b->rec_cap = capacity;
    return ISINGMC_OK;
}
int isingmc_record_count(const isingmc_batch *b, uint32_t *count, uint32_t *capacity) {
    if (!b) return ISINGMC_EINVAL;
    if (count) *count = b->rec_count;
    if (capacity) *capacity = b->rec_cap;
    return ISINGMC_OK;
}
int isingmc_record_clear(isingmc_batch *b) {
    if (!b) return ISINGMC_EINVAL;
    b->rec_count = 0;
    return ISINGMC_OK;
}
int isingmc_record_read(isingmc_batch *b, uint32_t first, uint32_t count, uint32_t r, uint8_t *out) {
    if (!b) return ISINGMC_EINVAL;
    if (!out || (r != UINT32_MAX && r >= b->dev.R)) { b->err = "bad replica index"; return ISINGMC_EINVAL; }
    if (const int rc = rec_range(b, first, count)) return rc;
    HIP_TRY(b, hipSetDevice(b->device));
    const uint32_t R = b->dev.R, N = b->dev.N, nw = b->dev.nwords;
    const uint32_t cnt = r == UINT32_MAX ? R : 1u, r0 = r == UINT32_MAX ? 0u : r;
    // in pieces of at most 16 Mi words: rows of the selected replicas (one replica's rows are R * nwords words apart)
    const size_t per_row = (size_t)cnt * nw;
    const uint32_t piece = (uint32_t)std::max<size_t>(1, ((size_t)1 << 24) / per_row);
    std::vector<uint32_t> w(std::min<size_t>(piece, count) * per_row);
    for (uint32_t t0 = 0; t0 < count; t0 += piece) {
        const uint32_t nt = count - t0 < piece ? count - t0 : piece;
        const uint32_t *src = b->rec.as<uint32_t>() + ((size_t)(first + t0) * R + r0) * nw;
        HIP_TRY(b, hipMemcpy2DAsync(w.data(), per_row * 4, src, (size_t)R * nw * 4, per_row * 4, nt, hipMemcpyDeviceToHost, b->stream));
        HIP_TRY(b, hipStreamSynchronize(b->stream));
        unpack_bits(w.data(), (size_t)nt * cnt, N, nw, out + (size_t)t0 * cnt * N);
    }
    return ISINGMC_OK;
}

int isingmc_record_series(isingmc_batch *b, uint32_t ngroups, const uint32_t *group_start, const uint32_t *group_vars, const uint8_t *group_flip,
                          uint32_t first, uint32_t count, uint32_t *out_bits) {
    if (!b) return ISINGMC_EINVAL;
    if (!out_bits) { b->err = "sample record: no output buffer"; return ISINGMC_EINVAL; }
    if (const int rc = rec_make_series(b, ngroups, group_start, group_vars, group_flip, first, count)) return rc;
    const size_t bytes = (size_t)b->dev.R * ngroups * ((count + 31u) / 32u) * 4;
    HIP_TRY(b, hipMemcpyAsync(out_bits, b->obs_series.as<void>(), bytes, hipMemcpyDeviceToHost, b->stream));
    HIP_TRY(b, hipStreamSynchronize(b->stream));
    return ISINGMC_OK;
}
int isingmc_record_autocorrelation(isingmc_batch *b, uint32_t ngroups, const uint32_t *group_start, const uint32_t *group_vars,
                                   uint32_t first, uint32_t count, double *out) {
    if (!b) return ISINGMC_EINVAL;
    if (!out) { b->err = "sample record: no output buffer"; return ISINGMC_EINVAL; }
    if (b->rec && 4 * (obs_autocorr_lds_words(count) + 2) > 4 * b->lds_total_words) {
        b->err = "sample record: a series of this many samples, twice, exceeds LDS (bit_autocorr_kernel keeps it there)";
        return ISINGMC_ENOTIMPL;
    }
    if (const int rc = rec_make_series(b, ngroups, group_start, group_vars, nullptr, first, count)) return rc;
    const size_t bytes = (size_t)b->dev.R * count * sizeof(double);
    if (const int rc = rec_grow(b, b->obs_out, bytes, "autocorrelations")) return rc;
    const hipError_t e = launch_bit_autocorr(b->stream, b->obs_series.as<uint32_t>(), b->dev.R, ngroups, count, b->obs_out.as<double>());
    if (e != hipSuccess) { b->err = std::string("bit_autocorr launch: ") + hipGetErrorString(e); return ISINGMC_ENODEVICE; }
    HIP_TRY(b, hipMemcpyAsync(out, b->obs_out.as<void>(), bytes, hipMemcpyDeviceToHost, b->stream));
    HIP_TRY(b, hipStreamSynchronize(b->stream));
    return ISINGMC_OK;
}

} // extern "C"
