"""csrc/hip_host.h — the owner of device memory (DevBuf) and the bit packing that both handles of the C ABI share — compiled by the host
compiler into a stand-alone program under the address and undefined-behaviour sanitizers.  The program defines the few entry points of
the HIP runtime that the header uses itself, over malloc: they count the live blocks and the synchronisations of every stream, log
the order of events, and can make the n-th allocation fail.  No device, nothing loaded into Python."""
import os
import shutil
import subprocess

import pytest

PROGRAM = r"""
#include "hip_host.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <set>
#include <string>
#include <utility>
#include <vector>

// ---- the runtime, over malloc ----
static std::set<void *> g_live;
static std::map<hipStream_t, int> g_syncs;
static std::string g_log;             // M = allocation, F = free, S = synchronisation, in order
static long g_mallocs = 0, g_frees = 0;
static long g_fail_at = -1;           // the allocation with this number (counted from g_mallocs) fails

extern "C" {
hipError_t hipMalloc(void **p, size_t bytes) {
    if (g_fail_at == g_mallocs++) { *p = nullptr; return hipErrorOutOfMemory; }
    *p = std::malloc(bytes ? bytes : 1);
    g_live.insert(*p);
    g_log += 'M';
    return hipSuccess;
}
hipError_t hipFree(void *p) {
    if (!p) return hipSuccess;
    if (!g_live.erase(p)) { std::printf("free of a block that is not live\n"); std::abort(); }
    std::free(p);
    ++g_frees;
    g_log += 'F';
    return hipSuccess;
}
hipError_t hipStreamSynchronize(hipStream_t s) { g_syncs[s]++; g_log += 'S'; return hipSuccess; }
const char *hipGetErrorString(hipError_t) { return "stand-in"; }
hipError_t hipGetDeviceCount(int *n) { *n = 1; return hipSuccess; }
hipError_t hipGetDevice(int *d) { *d = 0; return hipSuccess; }
hipError_t hipSetDevice(int) { return hipSuccess; }
hipError_t hipDeviceGetAttribute(int *v, hipDeviceAttribute_t, int) { *v = 0; return hipSuccess; }
hipError_t hipMemcpy(void *dst, const void *src, size_t n, hipMemcpyKind) { std::memcpy(dst, src, n); return hipSuccess; }
}

#define CHECK(c) do { if (!(c)) { std::printf("line %d: %s\n", __LINE__, #c); return 1; } } while (0)
static long live() { return (long)g_live.size(); }
static int total_syncs() { int n = 0; for (auto &kv : g_syncs) n += kv.second; return n; }
static hipStream_t stream(uintptr_t k) { return reinterpret_cast<hipStream_t>(k); }

static int scope() {
    {
        DevBuf a;
        CHECK(!a && a.bytes() == 0 && a.as<char>() == nullptr);
        CHECK(a.alloc(100) == hipSuccess);
        CHECK(a && a.bytes() == 100 && a.as<char>() != nullptr && live() == 1);
        a.as<char>()[99] = 1; // (the block is that large)
        CHECK(a.alloc(40) == hipSuccess); // a second alloc frees what was held
        CHECK(a.bytes() == 40 && live() == 1 && g_frees == 1);
        a.reset();
        CHECK(!a && a.bytes() == 0 && live() == 0 && g_frees == 2);
        a.reset(); // (nothing to free)
        CHECK(g_frees == 2);
        CHECK(a.alloc(8) == hipSuccess);
    }
    CHECK(live() == 0 && g_mallocs == 3 && g_frees == 3);
    return 0;
}

static int moves() {
    {
        DevBuf a;
        CHECK(a.alloc(64) == hipSuccess);
        void *p = a.as<void>();
        {
            DevBuf b(std::move(a));
            CHECK(!a && a.bytes() == 0 && a.as<void>() == nullptr);
            CHECK(b.as<void>() == p && b.bytes() == 64 && live() == 1);
            DevBuf c;
            CHECK(c.alloc(16) == hipSuccess && live() == 2);
            c = std::move(b); // the block c held goes, b is empty
            CHECK(!b && b.bytes() == 0 && c.as<void>() == p && c.bytes() == 64 && live() == 1 && g_frees == 1);
            a = std::move(c);
            CHECK(!c && a.as<void>() == p && live() == 1 && g_frees == 1);
        } // b and c are moved from: their destructors free nothing
        CHECK(live() == 1 && g_frees == 1);
    }
    CHECK(live() == 0 && g_mallocs == 2 && g_frees == 2);
    return 0;
}

static int vector_of_buffers() {
    const long n = 100;
    {
        std::vector<DevBuf> v;
        size_t cap = v.capacity();
        int regrowths = 0;
        for (long i = 0; i < n; ++i) {
            DevBuf q;
            CHECK(q.alloc(8 + (size_t)i) == hipSuccess);
            v.push_back(std::move(q));
            if (v.capacity() != cap) { cap = v.capacity(); ++regrowths; }
            CHECK(live() == i + 1 && g_frees == 0); // a reallocation moves the owners: nothing is freed, nothing twice
        }
        CHECK(regrowths >= 4);
        for (long i = 0; i < n; ++i) CHECK(v[i].bytes() == 8 + (size_t)i && v[i]);
    }
    CHECK(live() == 0 && g_mallocs == n && g_frees == n); // (a second free of a block aborts in hipFree)
    return 0;
}

static int reserve_keeps() {
    DevBuf a;
    CHECK(a.reserve(64, stream(1)) == hipSuccess); // an empty buffer: nothing to wait for
    CHECK(total_syncs() == 0 && a.bytes() == 64);
    void *p = a.as<void>();
    CHECK(a.reserve(64, stream(1)) == hipSuccess && a.reserve(10, stream(1)) == hipSuccess && a.reserve(0, stream(2)) == hipSuccess);
    CHECK(a.as<void>() == p && a.bytes() == 64 && total_syncs() == 0 && g_mallocs == 1 && g_frees == 0 && g_log == "M");
    a.reset();
    CHECK(live() == 0);
    return 0;
}

static int reserve_grows() {
    DevBuf a;
    CHECK(a.alloc(64) == hipSuccess);
    CHECK(a.reserve(65, stream(1)) == hipSuccess);
    CHECK(a && a.bytes() == 65 && live() == 1);
    a.as<char>()[64] = 1;
    CHECK(g_syncs[stream(1)] == 1 && total_syncs() == 1);             // the given stream, once
    CHECK(g_log == "MSFM" && g_mallocs == 2 && g_frees == 1);         // ... before the free, then a new block
    CHECK(a.reserve(4096, stream(2)) == hipSuccess);
    CHECK(g_syncs[stream(1)] == 1 && g_syncs[stream(2)] == 1 && g_log == "MSFMSFM" && a.bytes() == 4096);
    a.reset();
    CHECK(live() == 0);
    return 0;
}

static int reserve_fails() {
    DevBuf keep, a;
    CHECK(keep.alloc(32) == hipSuccess && a.alloc(64) == hipSuccess);
    const long before = live();
    g_fail_at = g_mallocs; // the next allocation
    CHECK(a.reserve(128, stream(1)) == hipErrorOutOfMemory);
    CHECK(!a && a.bytes() == 0 && a.as<void>() == nullptr);
    CHECK(live() == before - 1 && g_syncs[stream(1)] == 1 && g_log == "MMSF");
    CHECK(a.reserve(128, stream(1)) == hipSuccess); // later, with memory again (the buffer is empty: nothing to wait for)
    CHECK(a && a.bytes() == 128 && live() == before && total_syncs() == 1);
    g_fail_at = g_mallocs;
    DevBuf c;
    CHECK(c.alloc(8) == hipErrorOutOfMemory && !c && c.bytes() == 0 && live() == before);
    keep.reset(); a.reset();
    CHECK(live() == 0);
    return 0;
}

static int bits() {
    const uint32_t sizes[] = {1u, 31u, 32u, 33u, 65u};
    const uint8_t values[] = {0u, 1u, 0xFFu, 1u, 0u, 0u, 0xFFu};
    const size_t rows = 2;
    for (uint32_t N : sizes) {
        const uint32_t nw = (N + 31u) / 32u;
        std::vector<uint8_t> in(rows * N), out(rows * N, 0xAB);
        for (size_t i = 0; i < in.size(); ++i) in[i] = values[(i * 5 + N) % 7];
        in[N - 1] = 0xFF; in[rows * N - 1] = 0xFF; // the last variable of either row is up
        std::vector<uint32_t> w(rows * nw, 0xFFFFFFFFu); // (pack_bits overwrites)
        pack_bits(in.data(), rows, N, nw, w.data());
        for (size_t r = 0; r < rows; ++r) {
            for (uint32_t v = 0; v < N; ++v) CHECK(((w[r * nw + (v >> 5)] >> (v & 31u)) & 1u) == (in[r * N + v] ? 1u : 0u));
            if (N % 32u) CHECK((w[r * nw + nw - 1] >> (N % 32u)) == 0u); // the unused high bits of the last word
        }
        unpack_bits(w.data(), rows, N, nw, out.data());
        for (size_t i = 0; i < in.size(); ++i) CHECK(out[i] == (in[i] ? 1u : 0u)); // 0xFF comes back as 1
    }
    CHECK(g_mallocs == 0);
    return 0;
}

int main(int argc, char **argv) {
    const std::string which = argc > 1 ? argv[1] : "";
    int rc = 2;
    if (which == "scope") rc = scope();
    if (which == "moves") rc = moves();
    if (which == "vector") rc = vector_of_buffers();
    if (which == "reserve_keeps") rc = reserve_keeps();
    if (which == "reserve_grows") rc = reserve_grows();
    if (which == "reserve_fails") rc = reserve_fails();
    if (which == "bits") rc = bits();
    if (rc) return rc;
    if (live() != 0 || g_frees > g_mallocs) { std::printf("%ld blocks live at exit\n", live()); return 3; }
    std::printf("ok\n");
    return 0; // (the leak checker looks at what malloc still holds)
}
"""

CASES = ["scope", "moves", "vector", "reserve_keeps", "reserve_grows", "reserve_fails", "bits"]


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hipcc = os.path.realpath(shutil.which("hipcc") or "/opt/rocm/bin/hipcc")
    rocm_include = os.path.join(os.path.dirname(os.path.dirname(hipcc)), "include")
    d = tmp_path_factory.mktemp("host_buffers")
    src = d / "host_buffers_main.cpp"
    src.write_text(PROGRAM)
    exe = str(d / "host_buffers_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-D__HIP_PLATFORM_AMD__", "-isystem", rocm_include, "-I" + os.path.join(root, "isingmontecarlo_amd", "csrc"), str(src), "-o", exe])
    return exe


@pytest.mark.parametrize("case", CASES)
def test_host_buffers(program, case):
    p = subprocess.run([program, case], capture_output=True, text=True)
    assert p.returncode == 0 and p.stdout.strip() == "ok", p.stdout[-2000:] + p.stderr[-4000:]
