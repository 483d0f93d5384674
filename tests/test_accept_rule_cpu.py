"""csrc/sse_accept.h — the integer acceptance rule of the trimmed diagonal kernel — against the f64 expressions of the oracle's
ora_diagonal_update (`u01(o) * den < num` for an insert, `u01(o) * num < den` for a removal), compiled by the host compiler.
The kernel calls the same header, so this is the rule the GPU runs; the bound den <= 2^21 is the one below which the oracle's
f64 product is exact (above it the kernel keeps the f64 form)."""
import os
import subprocess

PROGRAM = r"""
#include "sse_accept.h"
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <initializer_list>

static double u01(uint32_t x) { return (double)x * (1.0 / 4294967296.0); } // oracle/sse_oracle_internal.h
static long ncases = 0;

static void check_insert(double num, uint32_t rr1, uint32_t den) {
    const bool want = u01(rr1) * (double)den < num;
    const bool got = sse_accept_insert(rr1, den, sse_accept_insert_const(num));
    ++ncases;
    if (want != got) {
        std::printf("insert differs: num=%.17g rr1=%u den=%u oracle=%d header=%d\n", num, rr1, den, (int)want, (int)got);
        std::exit(1);
    }
}
static void check_remove(double num, uint32_t rr1, int32_t den) {
    const bool want = u01(rr1) * num < (double)den;
    const bool got = sse_accept_remove(den, sse_accept_remove_threshold(rr1, num * (1.0 / 4294967296.0)));
    ++ncases;
    if (want != got) {
        std::printf("remove differs: num=%.17g rr1=%u den=%d oracle=%d header=%d\n", num, rr1, den, (int)want, (int)got);
        std::exit(1);
    }
}
static uint32_t clamp_u32(double x) { return x <= 0.0 ? 0u : (x >= 4294967295.0 ? 4294967295u : (uint32_t)x); }

static const uint32_t DENS[] = {1u, 2u, 3u, 1000u, (1u << 21) - 1u, 1u << 21};

static void check_weight(double num) {
    // a lane that is no candidate: never, whatever the operands
    for (uint32_t den : DENS) {
        if (sse_accept_insert(4294967295u, den, SSE_ACCEPT_NEVER_INSERT) || sse_accept_insert(0u, den, SSE_ACCEPT_NEVER_INSERT) ||
            sse_accept_remove((int32_t)den + 1, SSE_ACCEPT_NEVER_REMOVE)) {
            std::printf("a non-candidate was accepted: den=%u\n", den);
            std::exit(1);
        }
    }
    for (uint32_t den : DENS) {
        // insert: rr1 around the threshold num * 2^32 / den, and at both ends of its range
        const double thr = num * 4294967296.0 / (double)den;
        const uint32_t r0 = clamp_u32(std::floor(thr));
        for (int d = -2; d <= 2; ++d) {
            const int64_t r = (int64_t)r0 + d;
            if (r >= 0 && r <= 4294967295ll) check_insert(num, (uint32_t)r, den);
        }
        check_insert(num, 0u, den);
        check_insert(num, 4294967295u, den);
        // remove at the same operands (den + 1 is what a removal sees at the same n)
        for (uint32_t r : {0u, 1u, r0, 0x7FFFFFFFu, 0x80000000u, 4294967295u}) {
            check_remove(num, r, (int32_t)den);
            check_remove(num, r, (int32_t)den + 1);
        }
    }
    // remove: den at trunc(un) and +-1, for uniforms over the whole range
    for (uint32_t r : {0u, 1u, 2u, 77u, 65536u, 0x12345678u, 0x7FFFFFFFu, 0x80000000u, 0xDEADBEEFu, 4294967294u, 4294967295u}) {
        const double un = (double)r * (num * (1.0 / 4294967296.0));
        const int64_t t0 = un < 4294967296.0 ? (int64_t)un : 4294967296ll;
        for (int d = -2; d <= 2; ++d) {
            const int64_t t = t0 + d;
            if (t >= 1 && t <= (int64_t)(1u << 21) + 1) check_remove(num, r, (int32_t)t);
        }
        check_remove(num, r, 1);
        check_remove(num, r, (int32_t)(1u << 21) + 1);
        // ... and the uniform at which un crosses an integer den
        for (uint32_t den : DENS) {
            if (!(num > 0.0)) continue;
            const uint32_t rc = clamp_u32(std::floor((double)den * 4294967296.0 / num));
            for (int d = -2; d <= 2; ++d) {
                const int64_t rr = (int64_t)rc + d;
                if (rr >= 0 && rr <= 4294967295ll) check_remove(num, (uint32_t)rr, (int32_t)den);
            }
        }
    }
}

int main() {
    const double betas[] = {0.05, 1.0 / 3.0, 0.7, 1.0, 4.0, 16.0, 64.0, 4096.0, 1e5};
    const uint32_t nbs[] = {1u, 3u, 12u, 80u, 3072u, 12288u};
    const double ws[] = {0.0, 0.5, 1.0, 2.0, 0.3, 0.6, 1.7, 2.0 / 3.0};
    for (double beta : betas)
        for (uint32_t nb : nbs)
            for (double w : ws) check_weight(beta * (double)nb * w); // as the oracle forms it: (beta * Nb) * weight
    // pseudo-random weights over seven decades (LCG: the cases are the same on every run)
    uint64_t s = 0x9E3779B97F4A7C15ull;
    for (int i = 0; i < 300; ++i) {
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        const double m = 1.0 + (double)(s >> 11) * (1.0 / 9007199254740992.0);
        check_weight(m * std::pow(10.0, (double)(i % 8) - 2.0));
    }
    // num * 2^32 beyond 2^53 (not representable to the unit) and the clamps: num * 2^32 >= 2^63, num = 0
    for (double num : {2097152.0, 2097152.5, 3e6 + 1.0 / 3.0, 1e9 / 7.0, 2147483647.75, 2147483648.0, 4294967296.0, 1e12, 1e300, 0.0})
        check_weight(num);
    if (sse_accept_insert_const(0.0) != SSE_ACCEPT_NEVER_INSERT || sse_accept_insert_const(-1.0) != SSE_ACCEPT_NEVER_INSERT ||
        sse_accept_insert_const(2147483648.0) != 1ull || sse_accept_insert_const(1e300) != 1ull) {
        std::printf("clamp of the insert constant is off\n");
        return 1;
    }
    std::printf("%ld cases agree\n", ncases);
    return 0;
}
"""


def test_integer_rule_matches_the_oracle_expressions(tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = tmp_path / "accept.cpp"
    src.write_text(PROGRAM)
    exe = str(tmp_path / "accept")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror",
                           "-I" + os.path.join(root, "isingmontecarlo_amd", "csrc"), str(src), "-o", exe])
    p = subprocess.run([exe], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    ncases = int(p.stdout.split()[0])
    assert ncases > 100000, p.stdout
