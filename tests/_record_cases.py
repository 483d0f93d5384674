"""The sample record's kernels past their smallest launch: lengths, models and observable groups, chosen on the CPU.

record_series_kernel and bit_autocorr_kernel (csrc/sse_observe.hip.h, launched from observe.hip, driven by record.hip) change
their geometry with the series length T and the model's state words: whole waves for a quarter of the lags up to 1024 threads, one
pass per OBS_LAGS * OBS_MAX_THREADS lags beyond, 64 lanes striding over a state row of more than 64 words, and two refusals where
an image would exceed the workgroup's LDS.  This module restates those rules on the host, lists the lengths with the geometry
each must produce (tests/test_record_cases_cpu.py pins the table against the restated rule), the models and the group lists, and
holds the fast yardstick of the exact autocorrelation.  tests/test_gpu_sample_record_edges.py runs the device.

The constants are parsed out of csrc/sse_launch.h, never retyped.  Nothing here touches a device."""
import os
import re

import numpy as np

_CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "isingmontecarlo_amd", "csrc")


def _constants(path, prefix):
    """constexpr uint32_t NAME = <integer>; of one header -> {NAME: value} for the names that start with `prefix`."""
    with open(path) as f:
        found = re.findall(r"^\s*constexpr\s+uint32_t\s+(" + prefix + r"[A-Z0-9_]*)\s*=\s*(0[xX][0-9a-fA-F]+|\d+)[uU]?\s*;", f.read(), re.M)
    return {name: int(value, 0) for name, value in found}


K = _constants(os.path.join(_CSRC, "sse_launch.h"), "OBS_")
OBS_TILE, OBS_SERIES_WAVES, OBS_LAGS, OBS_MAX_THREADS = K["OBS_TILE"], K["OBS_SERIES_WAVES"], K["OBS_LAGS"], K["OBS_MAX_THREADS"]
LDS_WORDS = 160 * 1024 // 4   # a workgroup's LDS on gfx950, in words (isingmc_batch::lds_total_words)
READ_PIECE_WORDS = 1 << 24    # isingmc_record_read copies rows in pieces of at most this many words
ENOTIMPL, EINVAL = -5, -1


# ---- the launch rules of sse_launch.h / observe.hip / record.hip, restated ----
def nwords_of(nvars):
    return (int(nvars) + 31) // 32


def obs_row_stride(nwords):
    return nwords | 1


def obs_series_lds_words(nwords):
    return OBS_TILE * obs_row_stride(nwords)


def obs_autocorr_lds_words(tmax):
    return 2 * ((tmax + 31) // 32)


def series_accepted(nwords):
    """rec_make_series: the 64 staged state rows fit a workgroup's LDS."""
    return obs_series_lds_words(nwords) <= LDS_WORDS


def autocorr_accepted(tmax):
    """isingmc_record_autocorrelation: the series twice and the two counters fit a workgroup's LDS."""
    return obs_autocorr_lds_words(tmax) + 2 <= LDS_WORDS


def autocorr_geometry(tmax):
    """launch_bit_autocorr: (threads, passes of the kernel's lag0 loop)."""
    threads = min(((tmax + OBS_LAGS - 1) // OBS_LAGS + 63) // 64 * 64, OBS_MAX_THREADS)
    per_pass = threads * OBS_LAGS
    return threads, (tmax + per_pass - 1) // per_pass


def dead_lag_lanes(tmax):
    """Lanes of the last pass whose k-th lag (k = 0 .. OBS_LAGS - 1) lies beyond the series: [OBS_LAGS] counts."""
    threads, passes = autocorr_geometry(tmax)
    lag0 = (passes - 1) * threads * OBS_LAGS
    return [sum(1 for tid in range(threads) if lag0 + k * threads + tid >= tmax) for k in range(OBS_LAGS)]


def counting_waves(tmax):
    """bit_autocorr_kernel's staging loop counts the set bits of word j < Tw on lane j (and j + threads, ...): (waves that hold
    such a lane and so add to the shared counter, words of the busiest lane).  Up to T = 2048 (Tw <= 64) wave 0 counts alone,
    whatever the number of waves."""
    threads, _ = autocorr_geometry(tmax)
    tw = (tmax + 31) // 32
    return min((tw + 63) // 64, threads // 64), (tw + threads - 1) // threads


def series_tiles(tmax):
    return (tmax + OBS_TILE - 1) // OBS_TILE


def staging_trips(nwords):
    """Trips of record_series_kernel's staging loop `for (j = lane; j < nwords; j += 64)` for lane 0, and the lanes in the last."""
    trips = (nwords + 63) // 64
    return trips, nwords - 64 * (trips - 1)


# ---- lengths ----
# T -> (threads, passes) that launch_bit_autocorr must choose, and what the length is there for
AUTOCORR_LENGTHS = {
    256: (64, 1),      # the last single-wave length
    257: (128, 1),     # the first two-wave length (wave 1 takes lags and stages words, but counts none: counting_waves)
    1000: (256, 1),    # the 4th lag is dead for lanes >= 232
    2047: (512, 1),    # around a word end inside the multi-wave range
    2048: (512, 1),    # the last length whose set bits wave 0 counts alone (Tw = 64)
    2049: (576, 1),    # the first with two waves adding to one counter: wave 1 holds one word
    4095: (1024, 1),   # the full-size workgroup
    4096: (1024, 1),
    4097: (1024, 2),   # the second pass has one live lag
    8192: (1024, 2),   # two full passes
    8193: (1024, 3),
    16385: (1024, 5),
}
# Tw = 1025 words: all 16 waves add to the counter (Tw > 960) and lane 0 counts two words (Tw > 1024); nine passes.  The lengths
# above stop at nine counting waves, so this one runs too, on a record of its own and the few product observables.
AUTOCORR_LONGEST = (32769, (1024, 9))
AUTOCORR_FIRSTS = [0, 5]
AUTOCORR_SAMPLES =max(AUTOCORR_LENGTHS) + max(AUTOCORR_FIRSTS)
# the model of the autocorrelation cases: the 6x6 frustrated lattice of tests/test_gpu_sample_record.py (N = 36: the last state word
# is partial; couplings of both signs), R = 3, at beta = 0.4 instead of 1: at beta = 1 a replica's state repeats in one step of
# eight (every cluster keeps its value) and whole record rows repeat about 30 times in 16390; at 0.4 a replica repeats about 50
# times and a row never (test_record_cases_cpu checks it on the oracle's trajectory)
AUTOCORR_MODEL = dict(side=6, gamma=1.0, beta=0.4, cutoff=36, capacity=1 << 13, seed=2024, R=3)
# series lengths around tile (64) and word (32) ends; 4097 is 64 whole tiles and one sample
SERIES_LENGTHS = [63, 65, 95, 96, 97, 127, 128, 129]
SERIES_LONG = 4097
SERIES_FIRSTS = [0, 5]
SERIES_SAMPLES = max(SERIES_LENGTHS) + max(SERIES_FIRSTS)   # 134 >= 130 rows per model

# the two LDS boundaries: (largest accepted, first refused)
NWORDS_EDGE = (639, 640)
T_EDGE = (655328, 655329)


# ---- models ----
# name -> (N, R, seed, samples): periodic chains (tests/_lattices.chain with uni_chain couplings; N = 1 has no edge) at gamma = 1,
# beta = BETA, from one random state for all replicas.  At this beta a string holds about 0.2 N operators, so most spins are free
# in every step and are redrawn: every variable takes both values within a few samples and a recorded row ([R][N] bits) repeats
# with probability 2^-(free spins).  For N = 1, R = 5 that is 1/32 per step: the seed of that model is the first one (searched with
# the CPU oracle, whose trajectory the device's equals bit for bit) whose 134 rows never repeat; see check_rows.
BETA, GAMMA = 0.1, 1.0
MODELS = {
    "n1": (1, 5, 44, SERIES_SAMPLES),                     # one word, one bit of it (seed 44: the first of 0, 1, ... without a repeat)
    "n32": (32, 3, 11, SERIES_LONG + max(SERIES_FIRSTS)), # a full single word; the long series
    "n2048": (2048, 1, 12, SERIES_SAMPLES),               # nwords = 64, stride 65: exactly one staging trip of all 64 lanes
    "n2080": (2080, 5, 13, SERIES_SAMPLES),               # nwords = 65: the second trip has one lane
    "n20448": (20448, 3, 14, SERIES_SAMPLES),             # nwords = 639: 64 * 639 = 40896 of 40960 words, the largest accepted
}
REFUSED_MODEL = (20449, 1, 15)                            # nwords = 640, stride 641: 41024 words
ORACLE_MODEL = "n2080"                                    # the model whose recorded rows are compared with the oracle's replicas


def model_edges(nvars):
    import _lattices as lat
    return lat.chain(nvars, lat.uni_chain)


def model_capacity(nvars):
    """Slots of a replica's string: n ~ 0.25 N at BETA, the cutoff 1.5 n."""
    return max(64, 2 * nvars)


def initial_state(nvars, seed):
    return (np.random.default_rng(1000 + seed).random(nvars) < 0.5).astype(np.uint8)


# ---- observable groups ----
def edge_variables(nvars):
    """Variables next to the state words' ends: 0, 31, 32, 63, 64, the first bit of the last word and N - 1."""
    nw = nwords_of(nvars)
    return sorted({v for v in (0, 31, 32, 63, 64, 32 * (nw - 1), nvars - 1) if 0 <= v < nvars})


def many_groups(nvars, count=3001, seed=5):
    """`count` groups of one to three variables (drawn with repeats: a variable twice cancels)."""
    rng = np.random.default_rng(seed + nvars)
    sizes = rng.integers(1, 4, size=count)
    return [rng.integers(0, nvars, size=int(k)).tolist() for k in sizes]


def group_lists(nvars):
    """name -> (groups, indices of the groups that are constant by construction).  Launches with 1, 3, 4 and 5 groups leave waves
    of record_series_kernel idle or give one a second group; "many" gives every wave about 750."""
    ev = edge_variables(nvars)
    v, w = ev[-1], ev[0]
    lists = {
        "edges": ([[x] for x in ev], []),
        "one": ([[v]], []),
        "three": ([[v], [w, w], [w, w, v]], [1]),                          # [w, w] is the constant 0, [w, w, v] is [v]
        "four": ([[w], [v, v], [v, v, w], [v]], [1]),
        "constants_around": ([[v, v], [w], [v, v], [v], [w, w]], [0, 2, 4]),  # a constant before, between and after live series
        "many": (many_groups(nvars), None),
    }
    if nvars == 2080:
        lists["all"] = ([list(range(nvars)), [v]], [])                     # a group of all N variables
    if nvars == 1:
        lists["many"] = ([[0], [0, 0], [0, 0, 0]] * 1000 + [[0]], None)
    return lists


def constant_by_construction(groups):
    """Indices of the groups in which every variable occurs an even number of times."""
    out = []
    for i, g in enumerate(groups):
        vals, counts = np.unique(np.asarray(g), return_counts=True)
        if not (counts & 1).any():
            out.append(i)
    return out


def random_flips(ngroups, seed=9):
    return (np.random.default_rng(seed + ngroups).random(ngroups) < 0.5).astype(np.uint8)


def autocorr_observables(graph):
    """name -> groups on the 6x6 lattice of the autocorrelation tests: the reference's three kinds (variables, products, bonds),
    the products with duplicated variables and with constants before, between and after live series (cnt == 0 skips the
    atomicAdd of bit_autocorr_kernel while the other counter still has to be clear)."""
    from isingmontecarlo_amd.autocorrelations import variable_groups, bond_groups
    prods = [[7, 7], [0, 1], [2, 3, 4], [35, 35], [35], [1, 6, 7, 15], [3, 3, 9], [0, 31, 32, 33, 35], list(range(36)), [4, 4, 4, 4]]
    return {"variables": variable_groups(graph.nvars)[0], "products": prods, "bonds": bond_groups(graph)[0]}


# ---- the numpy side ----
def observe(states, groups, flips=None):
    """[T][n] of 0/1 from [T][N] states: parity of each group's bits ^ flip."""
    st = np.asarray(states, dtype=np.uint8)
    out = np.empty((st.shape[0], len(groups)), dtype=np.uint8)
    for i, vs in enumerate(groups):
        vs = np.asarray(vs, dtype=np.int64)
        out[:, i] = st[:, vs[0]] if len(vs) == 1 else np.bitwise_xor.reduce(st[:, vs], axis=1)
    if flips is not None:
        out ^= np.asarray(flips, dtype=np.uint8)[None, :]
    return out & 1


def pack_series(bits):
    """[T][n] of 0/1 -> uint32 [n][(T + 31) // 32], bit t & 31 of word t >> 5, padding bits 0 (record_series' layout)."""
    bits = np.asarray(bits, dtype=np.uint8)
    tmax, n = bits.shape
    tw = (tmax + 31) // 32
    padded = np.zeros((tw * 32, n), dtype=np.uint8)
    padded[:tmax] = bits
    by_byte = np.packbits(padded.T.reshape(n, tw, 4, 8), axis=3, bitorder="little").reshape(n, tw, 4).astype(np.uint32)
    return by_byte[:, :, 0] | (by_byte[:, :, 1] << 8) | (by_byte[:, :, 2] << 16) | (by_byte[:, :, 3] << 24)


def fast_bit_autocorrelation(bits):
    """autocorrelations.bit_autocorrelation with its O(T^2) loop replaced: the same integers, the same divisions in the same order,
    bit for bit the same result.  The Hamming distance of a 0/1 series b to its rotation by tau is
    ham = 2 ones - 2 sum_t b[t] b[(t + tau) mod T]; the circular correlation comes from one real FFT, irfft(|rfft b|^2), and is an
    integer below T, so it is rounded, and the distance to the nearest integer must stay below 0.25 for the rounding to be safe."""
    b = np.asarray(bits)
    if b.ndim != 2 or b.shape[0] == 0 or b.shape[1] == 0:
        raise ValueError("bits must be [T][n] with T, n >= 1")
    b = (b != 0)
    tmax, n = b.shape
    t = np.int64(tmax)
    ones = b.sum(axis=0, dtype=np.int64)
    f = np.fft.rfft(b.astype(np.float64), axis=0)
    corr = np.fft.irfft((f * np.conj(f)).real, n=tmax, axis=0)
    whole = np.rint(corr)
    assert np.abs(corr - whole).max() < 0.25, "the FFT's rounding error is too large to recover the integer correlations"
    ham = 2 * ones[None, :] - 2 * whole.astype(np.int64)
    s = 2 * ones - t
    den = t * t - s * s
    live = den != 0
    fden = np.where(live, den, 1).astype(np.float64)
    num = t * (t - 2 * ham) - (s * s)[None, :]
    acc = np.zeros(tmax, dtype=np.float64)
    for i in range(n):  # one division per term, terms added in observable order
        if live[i]:
            acc += num[:, i].astype(np.float64) / fden[i]
    return acc / np.float64(n)


def correlated_bits(seed, tmax, n, p_flip=0.1, constant=None):
    """[T][n] of 0/1: every column a two-state Markov chain (a flip with probability p_flip per step); column `constant` never
    changes (test_sample_record_cpu.correlated_bits)."""
    rng = np.random.default_rng(seed)
    flips = rng.random((tmax, n)) < p_flip
    flips[0] = rng.random(n) < 0.5
    if constant is not None:
        flips[1:, constant] = False
    return (np.cumsum(flips, axis=0) & 1).astype(np.uint8)


def check_rows(rows, what):
    """The condition on a case's recorded rows [T][R][N]: no record row equals the one before it (so neither does any window)."""
    rows = np.asarray(rows)
    same = (rows[1:] == rows[:-1]).reshape(rows.shape[0] - 1, -1).all(axis=1)
    assert not same.any(), f"{what}: record rows {np.flatnonzero(same)[:5] + 1} repeat the row before"


def check_series(series, constant, what):
    """The condition on a case's numpy series [T][n] of one replica: at least 90 % of the groups take both values, the groups
    `constant` (indices), which are constant by construction, excepted."""
    series = np.asarray(series)
    keep = np.setdiff1d(np.arange(series.shape[1]), np.asarray(constant, dtype=np.int64))
    if series.shape[0] > 1 and len(keep):
        both = (series[:, keep].min(axis=0) != series[:, keep].max(axis=0))
        assert both.sum() >= 0.9 * len(keep), f"{what}: only {int(both.sum())} of {len(keep)} groups take both values"
