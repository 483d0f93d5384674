"""csrc/sse_itime.h — the event identity behind isingmc_itime_groups — against the direct fold, in a stand-alone program built with
the host compiler under AddressSanitizer and UBSan.  The kernel (sse_itime.hip.h) calls the same header for every term it adds, so
this is the arithmetic the GPU runs; here it is driven sequentially, one event after the other.

The direct fold propagates a state through a random, consistent op-string and evaluates every group in front of every slot.  The
event form starts from the groups' bits at p = 0 and visits only the off-diagonal ops: per flipped variable and per group that lists
it, toggle the group's bit and add delta * weight.  Cases: empty strings, cutoffs 1, 63, 64, 65 and random ones, an event at slot 0
and at slot M - 1, groups hit twice by one op (both legs of a two-variable op), a variable listed twice in a group, strings with no
op at all and with every slot occupied."""
import os
import subprocess

PROGRAM = r"""
#include "sse_itime.h"
#include <cstdio>
#include <cstdlib>
#include <vector>

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd(uint32_t n) { // LCG: the same cases on every run
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)((rng_state >> 33) % n);
}

struct Model { uint32_t N; std::vector<int> a, c; }; // bond -> variables, c = -1 for a one-variable bond
struct Groups { std::vector<std::vector<uint32_t>> vars; std::vector<uint32_t> flip; };

static uint32_t group_bit(const Groups &G, size_t g, const std::vector<uint8_t> &st) {
    uint32_t par = G.flip[g];
    for (uint32_t v : G.vars[g]) par ^= st[v];
    return par & 1u;
}

// fill: 0 = no op at all, 1 = every slot occupied, 2 = random; force0 / forceLast: an off-diagonal op at slot 0 / M - 1
static std::vector<uint32_t> make_string(const Model &m, uint32_t M, std::vector<uint8_t> st, int fill, bool force0, bool forceLast, uint32_t *n_out,
                                         std::vector<uint8_t> *end_state) {
    std::vector<uint32_t> ops(M, 0u);
    uint32_t n = 0;
    for (uint32_t p = 0; p < M; ++p) {
        const bool forced = (force0 && p == 0) || (forceLast && p + 1 == M);
        if (fill == 0 || (fill == 2 && !forced && rnd(3) == 0)) continue;
        const uint32_t b = rnd((uint32_t)m.a.size());
        const bool two = m.c[b] >= 0;
        const uint32_t in = st[m.a[b]] | (two ? st[m.c[b]] << 1 : 0u);
        uint32_t fl = rnd(2) ? rnd(two ? 4u : 2u) : 0u; // half of the ops diagonal
        if (forced && !fl) fl = two ? 3u : 1u;
        const uint32_t out = in ^ fl;
        ops[p] = ((b + 1u) << 4) | in | (out << 2);
        st[m.a[b]] = out & 1u;
        if (two) st[m.c[b]] = (out >> 1) & 1u;
        ++n;
    }
    *n_out = n;
    *end_state = st;
    return ops;
}

static long ncases = 0, nevents = 0, ndouble = 0;

static void check(const Model &m, const Groups &G, uint32_t M, int fill, bool force0, bool forceLast) {
    std::vector<uint8_t> st0(m.N), st_end;
    for (auto &s : st0) s = (uint8_t)rnd(2);
    uint32_t n = 0;
    const std::vector<uint32_t> ops = make_string(m, M, st0, fill, force0, forceLast, &n, &st_end);
    const size_t ng = G.vars.size();
    // direct fold: every group in front of every slot
    std::vector<int64_t> want_all(ng, 0), want_occ(ng, 0);
    {
        std::vector<uint8_t> st = st0;
        for (uint32_t p = 0; p < M; ++p) {
            for (size_t g = 0; g < ng; ++g) {
                const int64_t x = sse_itime_value(group_bit(G, g, st));
                want_all[g] += x;
                if (ops[p]) want_occ[g] += x;
            }
            if (ops[p]) {
                const uint32_t b = (ops[p] >> 4) - 1u;
                st[m.a[b]] = (ops[p] >> 2) & 1u;
                if (m.c[b] >= 0) st[m.c[b]] = (ops[p] >> 3) & 1u;
            }
        }
    }
    // event form
    std::vector<uint32_t> bit(ng), bit0(ng);
    for (size_t g = 0; g < ng; ++g) bit[g] = bit0[g] = group_bit(G, g, st0);
    std::vector<int64_t> ev_all(ng, 0), ev_occ(ng, 0);
    uint32_t occ = 0;
    for (uint32_t p = 0; p < M; ++p) {
        if (!ops[p]) continue;
        ++occ;
        const uint32_t f = sse_itime_flips(ops[p]);
        const uint32_t b = (ops[p] >> 4) - 1u;
        const int64_t w_all = sse_itime_behind(M, p), w_occ = sse_itime_occupied_behind(n, occ);
        if (w_all < 0 || w_occ < 0) { std::printf("negative weight\n"); std::exit(1); }
        std::vector<int> hits(ng, 0);
        for (uint32_t leg = 0; leg < 2; ++leg) {
            if (!((f >> leg) & 1u)) continue;
            const uint32_t v = (uint32_t)(leg ? m.c[b] : m.a[b]);
            for (size_t g = 0; g < ng; ++g)
                for (uint32_t u : G.vars[g]) {
                    if (u != v) continue;
                    const int64_t d = sse_itime_delta(bit[g]);
                    bit[g] ^= 1u;
                    ev_all[g] += d * w_all;
                    ev_occ[g] += d * w_occ;
                    ++nevents;
                    if (++hits[g] == 2) ++ndouble;
                }
        }
    }
    for (size_t g = 0; g < ng; ++g) {
        const int64_t got_all = sse_itime_total(M, bit0[g], ev_all[g]), got_occ = sse_itime_total(n, bit0[g], ev_occ[g]);
        if (got_all != want_all[g] || got_occ != want_occ[g]) {
            std::printf("M=%u n=%u group %zu: all %lld vs %lld, occupied %lld vs %lld\n", M, n, g, (long long)got_all, (long long)want_all[g],
                        (long long)got_occ, (long long)want_occ[g]);
            std::exit(1);
        }
    }
    if ((fill == 0 && n != 0) || (fill == 1 && n != M)) { std::printf("fill is off\n"); std::exit(1); }
    ++ncases;
}

int main() {
    Model m;
    m.N = 7;
    for (uint32_t i = 0; i < m.N; ++i) { m.a.push_back((int)i); m.c.push_back((int)((i + 1) % m.N)); } // two-variable bonds (may flip one or both)
    for (uint32_t i = 0; i < m.N; ++i) { m.a.push_back((int)i); m.c.push_back(-1); }                    // one-variable bonds
    Groups G;
    for (uint32_t v = 0; v < m.N; ++v) { G.vars.push_back({v}); G.flip.push_back(0u); }
    for (uint32_t v = 0; v < m.N; ++v) { G.vars.push_back({v, (v + 1) % m.N}); G.flip.push_back(v & 1u); } // both legs of a bond: hit twice by one op
    G.vars.push_back({0, 1, 2, 3, 4, 5, 6}); G.flip.push_back(1u);
    G.vars.push_back({0, 3, 5}); G.flip.push_back(0u);
    G.vars.push_back({2, 2}); G.flip.push_back(0u);    // a variable listed twice: constant
    G.vars.push_back({2, 4, 2}); G.flip.push_back(1u); // ... and next to another one
    const uint32_t cutoffs[] = {0u, 1u, 2u, 63u, 64u, 65u, 127u, 128u, 129u, 1000u};
    for (uint32_t M : cutoffs)
        for (int fill = 0; fill < 3; ++fill)
            for (int force = 0; force < 4; ++force)
                for (int rep = 0; rep < 20; ++rep) check(m, G, M, fill, M > 0 && fill && (force & 1), M > 0 && fill && (force & 2));
    for (int rep = 0; rep < 300; ++rep) check(m, G, 1u + rnd(700u), 2, rnd(2) != 0, rnd(2) != 0);
    if (ndouble == 0) { std::printf("no op hit a group twice\n"); return 1; }
    std::printf("%ld cases agree, %ld events, %ld second hits\n", ncases, nevents, ndouble);
    return 0;
}
"""


def test_event_identity_matches_the_direct_fold(tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = tmp_path / "itime.cpp"
    src.write_text(PROGRAM)
    exe = str(tmp_path / "itime")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra", "-Werror",
                           "-I" + os.path.join(root, "isingmontecarlo_amd", "csrc"), str(src), "-o", exe])
    p = subprocess.run([exe], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    assert int(p.stdout.split()[0]) > 2000 and int(p.stdout.split()[3]) > 100000, p.stdout
