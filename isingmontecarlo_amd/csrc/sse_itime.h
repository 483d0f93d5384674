// sse_itime.h — the arithmetic of the imaginary-time fold of two-valued observables (isingmc_itime_groups) in exact integers.
//
// An observable x_g(p) = +-1 (a parity of state bits, sse_observe.hip.h) is constant between the off-diagonal ops that flip an odd
// number of its variables.  With M slots (the cutoff), n of them occupied, and the EVENTS of a group — one per flipped variable of
// the group, an op that flips two variables of it being two events at the same slot — taken in slot order:
//     sum over p < M of x(p)          =  M x(0) + sum over events of  delta * (M - 1 - p)
//     sum over occupied p of x(p)     =  n x(0) + sum over events of  delta * (occupied slots behind p)
// where delta = -2 x(just before the event): x(p) is the value BEFORE slot p's op, so an event at p changes the terms of the
// slots behind p and not its own.  Everything is an integer; |sum| <= M < 2^32, and the event terms stay below 2 M^2 < 2^63.
// Plain inline functions: compiled by hipcc for the kernel (sse_itime.hip.h) and by a host C++ compiler for
// tests/test_itime_rule_cpu.py (no HIP header needed).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SSE_ITIME_FN __host__ __device__ inline
#else
#define SSE_ITIME_FN inline
#endif

// the value of an observable from its bit (sse_observe.hip.h: 1 stands for +1)
SSE_ITIME_FN int64_t sse_itime_value(uint32_t bit) { return (bit & 1u) ? 1 : -1; }
// which of an op word's two variables it flips: bit 0 = relative variable 0, bit 1 = relative variable 1 (include/sse_format.h);
// 0 for an empty slot and for a diagonal op
SSE_ITIME_FN uint32_t sse_itime_flips(uint32_t word) { return (word ^ (word >> 2)) & 3u; }
// the step of an observable whose bit was bit_before when one of its variables flips
SSE_ITIME_FN int64_t sse_itime_delta(uint32_t bit_before) { return -2 * sse_itime_value(bit_before); }
// slots behind slot p of a string of M slots (p < M)
SSE_ITIME_FN int64_t sse_itime_behind(uint32_t M, uint32_t p) { return (int64_t)M - 1 - (int64_t)p; }
// occupied slots behind an occupied slot: n occupied in all, occ_upto of them at or before the slot (the slot itself included)
SSE_ITIME_FN int64_t sse_itime_occupied_behind(uint32_t n, uint32_t occ_upto) { return (int64_t)n - (int64_t)occ_upto; }
// the fold from the start bit and the accumulated event terms: count = M (all slots) or n (occupied slots)
SSE_ITIME_FN int64_t sse_itime_total(uint32_t count, uint32_t bit0, int64_t events) { return (int64_t)count * sse_itime_value(bit0) + events; }
