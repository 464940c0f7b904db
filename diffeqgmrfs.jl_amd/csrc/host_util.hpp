// Host-side plumbing shared by every handle of gmrf_hip.hip: the error state and its macros, device memory as objects that know
// their size and free themselves (DevBuf, DevArr<T>, reserve_group, HostWord), the carving of one allocation into pieces, a device
// context (device + stream) and the staging of host-resident arguments.  Self-contained; no kernels here.  Also env_int, the one
// reader of the integer GMRF_* environment switches.
//
// Ownership: a handle's device memory is a member of one of these types, so `delete` of the handle is the only free list.  A buffer
// is either OWNED (reserve: grow-only; freed on growth, release() and destruction) or BORROWED (borrow: the caller's memory, never
// freed).  Buffers that must never be half-present grow through reserve_group: all members or none.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include <algorithm>
#include <initializer_list>
#include <string>
#include <vector>

#include "../../include/gmrf_hip.h"

static thread_local std::string g_last_error;

#define HIPCHK(expr)                                                                        \
    do {                                                                                    \
        hipError_t _e = (expr);                                                             \
        if (_e != hipSuccess) {                                                             \
            g_last_error = std::string(#expr) + ": " + hipGetErrorString(_e);               \
            return GMRF_ERR_HIP;                                                            \
        }                                                                                   \
    } while (0)

#define GCHK(expr)                                                                          \
    do {                                                                                    \
        gmrf_status _s = (expr);                                                            \
        if (_s != GMRF_OK) return _s;                                                       \
    } while (0)

static gmrf_status bad_shape(const char* msg) {
    g_last_error = msg;
    return GMRF_ERR_BAD_SHAPE;
}

static bool is_device_ptr(const void* p) {
    if (!p) return false;
    hipPointerAttribute_t attr;
    hipError_t e = hipPointerGetAttributes(&attr, p);
    if (e != hipSuccess) {
        (void)hipGetLastError();   // unregistered host memory: clear the sticky error
        return false;
    }
    return attr.type == hipMemoryTypeDevice || attr.type == hipMemoryTypeManaged;
}

// Where DevBuf meets the device.  A stand-alone check of the ownership rules defines GMRF_HOST_UTIL_FAKE_DEVICE and its own three.
#ifndef GMRF_HOST_UTIL_FAKE_DEVICE
static hipError_t dev_alloc(void** p, size_t bytes) { return hipMalloc(p, bytes); }
static void dev_free(void* p) { (void)hipFree(p); }
static hipError_t dev_drain(hipStream_t stream) { return hipStreamSynchronize(stream); }
#endif

// An integer switch from the environment.  Callers keep the value in a function-local static: read once per process.
static int env_int(const char* name, int dflt) {
    const char* e = getenv(name);
    return e ? atoi(e) : dflt;
}

// Grow-only device buffer that frees itself.  What was enqueued on `stream` may still use the old allocation, so the stream is
// drained before it is freed.  A failed reserve leaves the buffer empty: the next call retries.
struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;                     // bytes
    bool owned = true;                  // false: p is the caller's (borrow), never freed

    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { release(); }

    bool fits(size_t bytes) const { return p && owned && bytes <= cap; }
    gmrf_status reserve(hipStream_t stream, size_t bytes) {
        if (fits(bytes)) return GMRF_OK;
        if (p && owned) HIPCHK(dev_drain(stream));
        release();
        bytes = std::max<size_t>(bytes, 16);
        if (hipError_t e = dev_alloc(&p, bytes); e != hipSuccess) {
            p = nullptr;
            g_last_error = std::string("hipMalloc (DevBuf::reserve): ") + hipGetErrorString(e);
            return GMRF_ERR_HIP;
        }
        cap = bytes;
        return GMRF_OK;
    }
    void borrow(void* q, size_t bytes) { release(); p = q; cap = bytes; owned = false; }
    void release() { if (p && owned) dev_free(p); p = nullptr; cap = 0; owned = true; }
    template <class T> T* as() const { return static_cast<T*>(p); }
};

// A member of a reserve_group: the buffer and the bytes it must hold.
struct Want { DevBuf* buf; size_t bytes; };

// Buffers that are used together grow together or not at all: if any member fails, every member is released.
static gmrf_status reserve_group(hipStream_t stream, std::initializer_list<Want> group) {
    gmrf_status s = GMRF_OK;
    for (const Want& w : group)
        if ((s = w.buf->reserve(stream, w.bytes)) != GMRF_OK) break;
    if (s != GMRF_OK)
        for (const Want& w : group) w.buf->release();
    return s;
}

// Typed DevBuf.  Converts to T*, so it stands wherever the raw pointer stood (arithmetic, null tests, kernel arguments).
template <class T> struct DevArr {
    DevBuf buf;

    operator T*() const { return static_cast<T*>(buf.p); }
    T* get() const { return static_cast<T*>(buf.p); }
    size_t size() const { return buf.cap / sizeof(T); }             // elements
    bool fits(size_t elems) const { return buf.fits(elems * sizeof(T)); }
    bool owned() const { return buf.owned; }
    gmrf_status reserve(hipStream_t stream, size_t elems) { return buf.reserve(stream, elems * sizeof(T)); }
    Want want(size_t elems) { return {&buf, elems * sizeof(T)}; }
    void borrow(T* q, size_t elems) { buf.borrow(q, elems * sizeof(T)); }
    void release() { buf.release(); }
    // Reserves and enqueues the copy of `elems` host elements; the caller keeps `src` alive until it has synchronised.
    gmrf_status upload(hipStream_t stream, const T* src, size_t elems) {
        GCHK(reserve(stream, elems));
        if (elems) HIPCHK(hipMemcpyAsync(buf.p, src, elems * sizeof(T), hipMemcpyHostToDevice, stream));
        return GMRF_OK;
    }
    gmrf_status upload(hipStream_t stream, const std::vector<T>& v) { return upload(stream, v.data(), v.size()); }
};

// One mapped host word (64 bytes) that a kernel writes and the host polls.
struct HostWord {
    unsigned* p = nullptr;

    HostWord() = default;
    HostWord(const HostWord&) = delete;
    HostWord& operator=(const HostWord&) = delete;
    ~HostWord() { if (p) (void)hipHostFree(p); }

    operator unsigned*() const { return p; }
    hipError_t open() {
        if (p) return hipSuccess;
        hipError_t e = hipHostMalloc(reinterpret_cast<void**>(&p), 64, hipHostMallocMapped);
        if (e == hipSuccess) *p = 0u; else p = nullptr;
        return e;
    }
};

// Device and stream of a handle.  device -1: the handle was created for its host side only (patterns); nothing of the
// GPU is touched, and ready() refuses the numeric calls.
struct DevCtx {
    int device = -1;
    hipStream_t stream = nullptr;
    bool own_stream = false;

    // Binds `dev` and the caller's stream, or creates one with `stream_flags`.  `who` prefixes a HIP failure.
    gmrf_status open(int32_t dev, void* user_stream, unsigned stream_flags, const char* who, bool pattern_only_ok = true) {
        if (dev < 0 && pattern_only_ok) return GMRF_OK;
        int count = 0;
        if (hipGetDeviceCount(&count) != hipSuccess || count <= 0 || dev < 0 || dev >= count) {
            (void)hipGetLastError();    // a failed count query leaves a sticky error
            g_last_error = "no HIP device visible (libgmrf_hip needs an MI355X / gfx950 GPU)";
            return GMRF_ERR_NO_DEVICE;
        }
        hipError_t e = hipSetDevice(dev);
        if (e == hipSuccess) {
            if (user_stream) stream = (hipStream_t)user_stream;
            else { e = hipStreamCreateWithFlags(&stream, stream_flags); own_stream = (e == hipSuccess); }
        }
        if (e != hipSuccess) { g_last_error = std::string(who) + ": " + hipGetErrorString(e); return GMRF_ERR_HIP; }
        device = dev;
        return GMRF_OK;
    }

    // Before a numeric call: `what` names the handle kind in the message of a pattern-only handle.
    gmrf_status ready(const char* what) const {
        if (device < 0) { g_last_error = std::string(what) + " (created with device -1)"; return GMRF_ERR_NO_DEVICE; }
        HIPCHK(hipSetDevice(device));
        return GMRF_OK;
    }

    bool has_device() const { return device >= 0; }

    // Drains the stream and destroys it if it is ours; the device stays selected for the caller's frees.
    void close() {
        if (!has_device()) return;
        (void)hipSetDevice(device);
        if (stream) (void)hipStreamSynchronize(stream);
        if (own_stream) (void)hipStreamDestroy(stream);
        stream = nullptr; own_stream = false;
    }
};

// The host-or-device arguments of ONE call.  in() / out() register an argument and where its device address goes;
// commit() sizes the handle's arena once for the call, fills in the addresses and uploads the host inputs; after the
// kernels, flush() brings the host outputs back.  A null pointer stays null, a device pointer passes through
// untouched, a host array gets a 16-byte aligned slice of the arena.  Nothing but the arena's capacity outlives the call.
struct Staging {
    struct Item { void* user; size_t bytes; void** dev; bool out; void* slice; };      // slice: its place in the arena, null if none
    DevBuf& arena;
    Item items[8];
    int count = 0;
    bool overflow = false;

    explicit Staging(DevBuf& a) : arena(a) {}

    template <class T> void in(const T* p, size_t bytes, const T** dev) { add(const_cast<T*>(p), bytes, (void**)dev, false); }
    template <class T> void out(T* p, size_t bytes, T** dev) { add(p, bytes, (void**)dev, true); }

    gmrf_status commit(hipStream_t stream) {
        if (overflow) return bad_shape("too many staged arguments");
        bool host[8];
        size_t need = 0;
        for (int i = 0; i < count; ++i) {
            host[i] = items[i].user && !is_device_ptr(items[i].user);
            if (host[i]) need += padded(items[i].bytes);
        }
        if (need) GCHK(arena.reserve(stream, need));
        size_t off = 0;
        for (int i = 0; i < count; ++i) {
            Item& it = items[i];
            if (!host[i]) { *it.dev = it.user; continue; }
            *it.dev = it.slice = arena.as<char>() + off;
            off += padded(it.bytes);
            if (!it.out) HIPCHK(hipMemcpyAsync(it.slice, it.user, it.bytes, hipMemcpyHostToDevice, stream));
        }
        return GMRF_OK;
    }

    gmrf_status flush(hipStream_t stream) {
        for (int i = 0; i < count; ++i)
            if (items[i].out && items[i].slice)
                HIPCHK(hipMemcpyAsync(items[i].user, items[i].slice, items[i].bytes, hipMemcpyDeviceToHost, stream));
        return GMRF_OK;
    }

    // what an item of `bytes` takes of the arena (a caller that sizes the arena ahead of commit() sums this)
    static size_t padded(size_t bytes) { return (bytes + 15) & ~(size_t)15; }

private:
    void add(void* p, size_t bytes, void** dev, bool out) {
        if (count == (int)(sizeof(items) / sizeof(items[0]))) { overflow = true; return; }
        items[count++] = {p, bytes, dev, out, nullptr};
    }
};

// Lays the pieces of one allocation out behind `base`, each 16-byte aligned and never empty.  A layout runs twice over the same
// list: with a null base for the size alone (no piece is written), then with the buffer.
struct Carve {
    char* base;
    size_t used = 0;
    template <class T> void operator()(T** piece, int64_t elems) {
        if (base) *piece = reinterpret_cast<T*>(base + used);
        used += Staging::padded(sizeof(T) * (size_t)std::max<int64_t>(elems, 1));
    }
};
