// sse_accept.h — the Metropolis acceptance rule of the diagonal sweep in exact integer arithmetic.
//
// The oracle (ora_diagonal_update; qmc_traits/diagonal.rs:142-191) decides with one uniform u = rr1 * 2^-32, rr1 a 32-bit
// Philox output, a weight num = beta * Nb * w and the integer den = M - n (insert) or M - n + 1 (remove):
//     insert iff  u * den < num          remove iff  u * num < den
// Both are statements about integers once den is one:
//   * insert:  rr1 * den < num * 2^32  <=>  rr1 * den < NBI,  NBI = ceil(num * 2^32)  (the left side is an integer), i.e. the
//     sign bit of rr1 * den + (2^63 - NBI) is clear: one 32 x 32 + 64 multiply-add and a sign test.  The oracle's f64 product
//     is exact only while rr1 * den < 2^53, so the two agree for den <= 2^21 (SSE_ACCEPT_MAX_DEN) and the callers keep the f64
//     form for longer strings;
//   * remove:  un < den  <=>  den > trunc(un)  with  un = (double)rr1 * (num * 2^-32)  rounded as the oracle rounds it (the
//     power of two moves between the factors exactly); the truncation saturates at INT32_MAX, which means "never" and is right:
//     den < 2^31.
// A slot that is no candidate gets the constant 2^63 (never inserted) or the threshold INT32_MAX (never removed), so the two
// comparisons give the accepted masks themselves.
// Plain inline functions: compiled by hipcc for the kernels (sse_fast.hip.h) and by a host C++ compiler for
// tests/test_accept_rule_cpu.py (no HIP header needed).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SSE_ACCEPT_FN __host__ __device__ inline
#else
#define SSE_ACCEPT_FN inline
#endif

#define SSE_ACCEPT_MAX_DEN (1u << 21)                 // integer and f64 rules agree for cutoffs up to here
#define SSE_ACCEPT_NEVER_INSERT 0x8000000000000000ull // 2^63: the sign bit stays set whatever rr1 * den (< 2^63) is
#define SSE_ACCEPT_NEVER_REMOVE 0x7FFFFFFF

// 2^63 - ceil(num * 2^32), ceil clamped to [0, 2^63 - 1]:  num <= 0 -> 2^63 (never), num * 2^32 >= 2^63 -> 1 (always)
SSE_ACCEPT_FN uint64_t sse_accept_insert_const(double num) {
    const double s = num * 4294967296.0; // exact
    if (!(s > 0.0)) return SSE_ACCEPT_NEVER_INSERT;
    if (s >= 9223372036854775808.0) return 1ull;
    uint64_t nbi = (uint64_t)s; // s < 2^63: in range; truncates
    if ((double)nbi < s) nbi += 1ull; // ceil ((double)nbi is exact: nbi has the 53 significant bits of s at most)
    return SSE_ACCEPT_NEVER_INSERT - nbi;
}

// insert candidate with constant c = sse_accept_insert_const(num):  u * den < num
SSE_ACCEPT_FN bool sse_accept_insert(uint32_t rr1, uint32_t den, uint64_t c) {
    return (int32_t)(((uint64_t)rr1 * (uint64_t)den + c) >> 32) >= 0;
}

// trunc(un) saturated to INT32_MAX, un = (double)rr1 * num_lo with num_lo = num * 2^-32 (un >= 0)
SSE_ACCEPT_FN int32_t sse_accept_remove_threshold(uint32_t rr1, double num_lo) {
    const double un = (double)rr1 * num_lo;
#if defined(__HIP_DEVICE_COMPILE__)
    int32_t r;
    asm("v_cvt_i32_f64 %0, %1" : "=v"(r) : "v"(un)); // truncates and saturates
    return r;
#else
    if (!(un < 2147483647.0)) return SSE_ACCEPT_NEVER_REMOVE;
    return un > 0.0 ? (int32_t)un : 0;
#endif
}

// removal candidate with threshold thr = sse_accept_remove_threshold(rr1, num * 2^-32):  u * num < den
SSE_ACCEPT_FN bool sse_accept_remove(int32_t den, int32_t thr) { return den > thr; }
