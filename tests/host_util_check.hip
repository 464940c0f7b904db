// Stand-alone check of the ownership rules of csrc/host_util.hpp (DevBuf, DevArr, reserve_group) without a device: the three
// allocation hooks are backed by malloc / free, a count of live allocations and a "fail the k-th allocation" knob.  Built with
// the host side under AddressSanitizer + UBSan by tests/test_host_util_cpu.py and run as a child process: a double free or an
// access out of bounds is the sanitizer's to report, a leak is the live count's.  Exit status 0: every rule held.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <set>
#include <type_traits>

#define GMRF_HOST_UTIL_FAKE_DEVICE
static std::set<void*> g_live;          // allocations handed out and not yet freed
static int g_allocs = 0, g_frees = 0, g_drains = 0;
static int g_fail_at = 0;               // fail the k-th allocation from now (1-based); 0: none
static int g_failures = 0;

static hipError_t dev_alloc(void** p, size_t bytes) {
    if (g_fail_at > 0 && --g_fail_at == 0) { *p = nullptr; return hipErrorOutOfMemory; }
    if (bytes == 0) { fprintf(stderr, "FAIL: allocation of zero bytes\n"); ++g_failures; }
    *p = malloc(bytes);
    memset(*p, 0xab, bytes);            // (touch all of it: the sanitizer sees the extent)
    g_live.insert(*p);
    ++g_allocs;
    return hipSuccess;
}
static void dev_free(void* p) {
    if (!g_live.erase(p)) { fprintf(stderr, "FAIL: free of %p, which is not a live allocation\n", p); ++g_failures; return; }
    free(p);
    ++g_frees;
}
static hipError_t dev_drain(hipStream_t) { ++g_drains; return hipSuccess; }

#include "../diffeqgmrfs.jl_amd/csrc/host_util.hpp"

#define CHECK(cond)                                                                         \
    do {                                                                                    \
        if (!(cond)) { fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); ++g_failures; } \
    } while (0)

static_assert(!std::is_copy_constructible<DevBuf>::value && !std::is_copy_assignable<DevBuf>::value, "DevBuf must not copy");
static_assert(!std::is_copy_constructible<DevArr<double>>::value && !std::is_copy_assignable<DevArr<double>>::value, "DevArr must not copy");
static_assert(!std::is_copy_constructible<HostWord>::value, "HostWord must not copy");

struct Counters { int allocs, frees, drains; };
static Counters now() { return {g_allocs, g_frees, g_drains}; }

struct Trio { DevArr<double> a; DevArr<int> b; DevArr<uint16_t> c; };
static gmrf_status grow(Trio& t, size_t n) { return reserve_group(nullptr, {t.a.want(n), t.b.want(2 * n), t.c.want(3 * n)}); }

static void failed_reserve() {
    DevArr<double> a;
    g_fail_at = 1;
    CHECK(a.reserve(nullptr, 100) == GMRF_ERR_HIP);
    CHECK(!a && a.size() == 0 && g_live.empty());
    CHECK(a.reserve(nullptr, 100) == GMRF_OK);
    CHECK(a && a.size() >= 100 && g_live.size() == 1);
    // ... and the same when the failure is that of a growth: the old allocation is gone, the array empty, nothing stale
    g_fail_at = 1;
    CHECK(a.reserve(nullptr, 1000) == GMRF_ERR_HIP);
    CHECK(!a && a.size() == 0 && !a.fits(1) && g_live.empty());
    CHECK(a.reserve(nullptr, 50) == GMRF_OK && a.size() >= 50);
    // never zero bytes
    DevArr<int> z;
    CHECK(z.reserve(nullptr, 0) == GMRF_OK && z);
    std::vector<int> none;
    CHECK(z.upload(nullptr, none) == GMRF_OK);
}

static void group_all_or_nothing() {
    for (int k = 1; k <= 3; ++k) {
        Trio t;
        g_fail_at = k;
        CHECK(grow(t, 10) == GMRF_ERR_HIP);
        CHECK(!t.a && !t.b && !t.c);
        CHECK(t.a.size() == 0 && t.b.size() == 0 && t.c.size() == 0);
        CHECK(g_live.empty());
        CHECK(g_fail_at == 0);
        CHECK(grow(t, 10) == GMRF_OK);
        CHECK(t.a && t.b && t.c && t.a.size() >= 10 && t.b.size() >= 20 && t.c.size() >= 30 && g_live.size() == 3);
        // a failed growth of a full group empties it too: the next call retries
        g_fail_at = k;
        CHECK(grow(t, 100) == GMRF_ERR_HIP);
        CHECK(!t.a && !t.b && !t.c && g_live.empty());
        CHECK(grow(t, 100) == GMRF_OK && g_live.size() == 3);
    }
    CHECK(g_live.empty());
}

static void growth() {
    DevArr<double> a;
    Counters c0 = now();
    CHECK(a.reserve(nullptr, 8) == GMRF_OK);
    CHECK(g_allocs == c0.allocs + 1 && g_frees == c0.frees && g_drains == c0.drains);     // (nothing to drain for: nothing to free)
    double* first = a;
    c0 = now();
    CHECK(a.reserve(nullptr, 8) == GMRF_OK && a.reserve(nullptr, 3) == GMRF_OK);          // not growing: neither
    CHECK(a.get() == first && g_allocs == c0.allocs && g_frees == c0.frees && g_drains == c0.drains);
    CHECK(a.reserve(nullptr, 64) == GMRF_OK);                                             // growing: one drain, then one free
    CHECK(g_allocs == c0.allocs + 1 && g_frees == c0.frees + 1 && g_drains == c0.drains + 1);
    CHECK(a.size() >= 64 && g_live.size() == 1 && !g_live.count(first));
    a[63] = 1.0;                                                                          // (host memory here: in bounds)
    c0 = now();
    a.release();
    CHECK(!a && a.size() == 0 && g_frees == c0.frees + 1 && g_live.empty());
    a.release();
    CHECK(g_frees == c0.frees + 1);
}

static void borrowed() {
    double* mine = static_cast<double*>(malloc(sizeof(double) * 32));
    double* mine2 = static_cast<double*>(malloc(sizeof(double) * 32));
    Counters c0 = now();
    {
        DevArr<double> a;
        a.borrow(mine, 32);
        CHECK(a.get() == mine && a.size() == 32 && !a.owned());
        a.borrow(mine2, 32);                               // replacing borrowed with borrowed
        CHECK(a.get() == mine2);
        a.release();                                       // release()
        CHECK(!a && a.owned());
        a.borrow(mine, 32);
        CHECK(a.reserve(nullptr, 4) == GMRF_OK);           // borrowed -> owned: nothing freed, our memory is ours
        CHECK(a.owned() && a.get() != mine && g_live.size() == 1);
        CHECK(g_frees == c0.frees && g_drains == c0.drains);
        a.borrow(mine2, 32);                               // owned -> borrowed: exactly the owned one is freed
        CHECK(g_frees == c0.frees + 1 && g_live.empty() && a.get() == mine2);
    }                                                      // destruction
    CHECK(g_frees == c0.frees + 1 && g_live.empty());
    mine[31] = mine2[31] = 3.0;                            // still ours (the sanitizer would object to a use after free)
    free(mine); free(mine2);
}

struct Handle {                         // a handle: `delete` is its only free list
    DevArr<double> a, b;
    DevArr<int> c;
    DevBuf arena;
    DevArr<double> theirs;
};

static void struct_of_arrays() {
    double* mine = static_cast<double*>(malloc(sizeof(double) * 4));
    Handle* h = new Handle();
    CHECK(h->a.reserve(nullptr, 10) == GMRF_OK && h->c.reserve(nullptr, 10) == GMRF_OK && h->arena.reserve(nullptr, 100) == GMRF_OK);
    h->theirs.borrow(mine, 4);
    std::vector<double> v(17, 1.5);
    CHECK(h->b.reserve(nullptr, v.size()) == GMRF_OK);
    CHECK(g_live.size() == 4);
    delete h;
    CHECK(g_live.empty());
    free(mine);
}

int main() {
    failed_reserve();
    group_all_or_nothing();
    growth();
    borrowed();
    struct_of_arrays();
    CHECK(g_live.empty());
    CHECK(g_allocs == g_frees);
    if (g_failures) { fprintf(stderr, "%d check(s) failed\n", g_failures); return 1; }
    printf("host_util_check: ok (%d allocations, %d drains)\n", g_allocs, g_drains);
    return 0;
}
