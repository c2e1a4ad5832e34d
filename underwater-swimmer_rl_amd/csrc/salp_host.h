// salp_host.h — host-only support shared by the two C ABI files, salp_vec.hip and salp_robot.hip: the error string and
// HIP_TRY, DeviceScope, the device-id check of the create calls, the frame every call on a handle opens with (CallFrame),
// launch_1d() and the one body that serves the host-pointer and the device-pointer form of a call (StageBuffer,
// HostStream, staged()).  The policy object of both files builds on it (salp_policy_object.h, included after this
// header).  Everything here has internal linkage, so each of the two translation units has an
// error string of its own (salp_last_error and salp_robot_last_error stay independent).  No device code; the rollout
// kernel units do not include it.  What the two files refuse is decided in headers that do not know fail() and compile
// without HIP (salp_params.h, salp_policy.h, salp_robot_params.h); the ABI file hands the reason to fail().
#ifndef SALP_HOST_H
#define SALP_HOST_H

#include <hip/hip_runtime.h>
#include <stddef.h>

#include <string>

#include "../../include/salp_vec.h"   // SALP_OK, SALP_ERR_*

namespace {

thread_local std::string g_err;
int fail(int code, const std::string& msg) { g_err = msg; return code; }

#define HIP_TRY(expr)                                                                              \
  do {                                                                                             \
    hipError_t _e = (expr);                                                                        \
    if (_e != hipSuccess)                                                                          \
      return fail(_e == hipErrorOutOfMemory ? SALP_ERR_OOM : SALP_ERR_HIP,                         \
                  std::string(#expr) + ": " + hipGetErrorString(_e));                              \
  } while (0)


// Makes `device` current for the scope of one ABI call and restores the caller's device afterwards, so that the
// library never changes the current HIP device under the caller (PyTorch keeps its own notion of it).  When the
// caller is already on the handle's device — the usual case — this is one hipGetDevice.
struct DeviceScope {
  int prev = -1, changed = 0;
  hipError_t enter(int device) {
    hipError_t e = hipGetDevice(&prev);
    if (e != hipSuccess) return e;
    if (prev != device) { e = hipSetDevice(device); changed = (e == hipSuccess); }
    return e;
  }
  ~DeviceScope() { if (changed) (void)hipSetDevice(prev); }
};

// What a create call checks before it touches `device_id`.
int check_device_id(int device_id) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    return fail(SALP_ERR_NO_DEVICE, "no HIP device visible (this library has no CPU fallback)");
  if (device_id < 0 || device_id >= ndev) return fail(SALP_ERR_NO_DEVICE, "device_id out of range");
  return SALP_OK;
}

// The opening of an ABI call on a handle: the handle's device is current for the frame's scope, `st` is the caller's
// stream, and a handle that keeps a `last_stream` (the snake handle; the robot handle has none) records it.
template <class Handle> auto record_stream(Handle* h, hipStream_t st, int) -> decltype((void)(h->last_stream = st)) { h->last_stream = st; }
template <class Handle> void record_stream(Handle*, hipStream_t, long) {}
struct CallFrame {
  DeviceScope dev_scope;
  hipStream_t st = nullptr;
  template <class Handle> int enter(Handle* h, void* stream) {
    HIP_TRY(dev_scope.enter(h->device));
    st = (hipStream_t)stream;
    record_stream(h, st, 0);
    return SALP_OK;
  }
};

inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// One thread per element: `kernel` over n elements in workgroups of `block` threads on `st`, and the launch's status.
inline unsigned blocks_for(int64_t n, int block) { return (unsigned)((n + block - 1) / block); }
template <class... Params, class... Args>
int launch_1d(void (*kernel)(Params...), int64_t n, int block, hipStream_t st, const Args&... args) {
  hipLaunchKernelGGL(kernel, dim3(blocks_for(n, block)), dim3(block), 0, st, args...);
  HIP_TRY(hipGetLastError());
  return SALP_OK;
}

// Device memory for the host-pointer calls, grown on demand.  `shrink` (the robot handle): a block over 64 MiB is also
// given up when a call needs less than a quarter of it — a history step with host pointers can stage gigabytes, the
// plain step after it a few megabytes.  Every host-pointer call ends with a stream synchronisation, so the old block is
// idle when it is released.  The owner is on the block's device when it calls ensure() and when the block goes.
struct StageBuffer {
  void* p = nullptr;
  size_t bytes = 0;
  bool shrink = false;
  int ensure(size_t need) {
    if (need <= bytes && !(shrink && bytes > ((size_t)64 << 20) && need < bytes / 4)) return SALP_OK;
    if (p) { (void)hipFree(p); p = nullptr; bytes = 0; }
    if (need == 0) return SALP_OK;
    const hipError_t e = hipMalloc(&p, need);   // (the message keeps the text it has always had)
    if (e != hipSuccess)
      return fail(e == hipErrorOutOfMemory ? SALP_ERR_OOM : SALP_ERR_HIP, std::string("hipMalloc(&h->stage, bytes): ") + hipGetErrorString(e));
    bytes = need;
    return SALP_OK;
  }
  StageBuffer() = default;
  StageBuffer(const StageBuffer&) = delete;
  StageBuffer& operator=(const StageBuffer&) = delete;
  ~StageBuffer() { if (p) (void)hipFree(p); }
};

// One stream of a host-pointer call: `count` elements at `host` (NULL = the stream is absent), copied to the device before
// the launch (kIn), back after it (kOut) or both.  staged() fills in `dev`, NULL for an absent stream.  A scratch piece
// (dir 0) has no host side: it is always present and copied in neither direction.
enum { kIn = 1, kOut = 2 };
struct HostStream {
  void* host; size_t bytes; int dir;
  void* dev;
  bool present() const { return host || dir == 0; }
  template <class T> T* as() const { return static_cast<T*>(dev); }
};
template <class T> HostStream stream_in(const T* p, size_t count) { return {const_cast<T*>(p), count * sizeof(T), kIn, nullptr}; }
template <class T> HostStream stream_out(T* p, size_t count, bool also_in = false) { return {p, count * sizeof(T), also_in ? kIn | kOut : kOut, nullptr}; }
inline HostStream stream_scratch(size_t bytes) { return {nullptr, bytes, 0, nullptr}; }

// The host-pointer form of a call, synchronous: the streams that are present get 256-byte-aligned pieces of the staging
// block `b`, the kIn ones are copied in, `launch` enqueues the call's kernels on the device pointers — a failure there
// ends the call — then the kOut ones are copied out and the stream is waited for.  The pieces stay where they are until
// the next call on `b`.
// `device_ptrs`: the caller's pointers are device pointers.  Each stream's `dev` is then the caller's pointer and `launch`
// is all there is: nothing is allocated, copied or waited for (such a call can be captured into a graph), `b` is not touched.
template <int N, class Launch>
int staged(StageBuffer& b, hipStream_t st, bool device_ptrs, HostStream (&s)[N], Launch&& launch) {
  if (device_ptrs) {
    for (HostStream& x : s) x.dev = x.host;
    return launch();
  }
  size_t need = 0;
  for (const HostStream& x : s)
    if (x.present()) need = align_up(need, 256) + x.bytes;
  int rc = b.ensure(need);
  if (rc != SALP_OK) return rc;
  size_t off = 0;
  for (HostStream& x : s) {
    if (!x.present()) continue;
    off = align_up(off, 256);
    x.dev = (char*)b.p + off;
    off += x.bytes;
    if (x.dir & kIn) HIP_TRY(hipMemcpyAsync(x.dev, x.host, x.bytes, hipMemcpyHostToDevice, st));
  }
  rc = launch();
  if (rc != SALP_OK) return rc;
  for (const HostStream& x : s)
    if (x.host && (x.dir & kOut)) HIP_TRY(hipMemcpyAsync(x.host, x.dev, x.bytes, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  return SALP_OK;
}

}  // namespace

#endif  // SALP_HOST_H
