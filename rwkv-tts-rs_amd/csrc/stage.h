// stage.h -- the host scaffold of a windowed audio stage behind the vocoder (resample.hip, tsm.hip):
// an object with one stream, one event pair, one read-only table and grow-only device buffers, that
// runs ragged windows of host PCM through its kernels in one call. A stage includes this and writes
// its kernels, its plan and its descriptor builder; everything here is host code, used directly (no
// virtual dispatch), and holds no floating-point arithmetic of its own.
#pragma once
#include <algorithm>
#include <initializer_list>
#include <mutex>
#include <new>
#include <vector>

#include "common.h"

namespace rwkvtts {

// Grow-only device array: nothing happens while want <= cap; otherwise the old array is freed first
// and want + want / 4 elements are allocated. cap is 0 if that allocation fails.
template <typename T>
struct DevBuf {
  T* p = nullptr;
  size_t cap = 0;
  int reserve(size_t want) {
    if (want <= cap) return RWKVTTS_OK;
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
    const size_t n = want + want / 4;
    RT_HIP(hipMalloc(&p, n * sizeof(T)));
    cap = n;
    return RWKVTTS_OK;
  }
};

// What every stage object holds; the stage's own struct derives from it. Desc is the per-workgroup
// descriptor its kernels read (one array per call, built on the host under mu). Out and Tab: the
// element types of the outputs and of the table, f32 for every stage but the FLAC encoder (flac.hip),
// whose outputs are bytes and whose table is int32.
template <typename Desc, typename Out = float, typename Tab = float>
struct Stage {
  int device = 0;
  Tab* d_table = nullptr;
  DevBuf<float> d_in;   // the windows' inputs, back to back
  DevBuf<Out> d_out;    // the windows' outputs, back to back
  DevBuf<Desc> d_desc;
  hipStream_t stream = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;  // bracket the kernels of a call, not its copies
  double kernel_ms = 0.0;
  std::mutex mu;  // one call at a time
  std::vector<Desc> desc;
};

// Frees whatever exists (extra: the stage's further device arrays) and the object.
template <typename S>
static void stage_free(S* s, std::initializer_list<void*> extra = {}) {
  if (s->d_table) (void)hipFree(s->d_table);
  if (s->d_in.p) (void)hipFree(s->d_in.p);
  if (s->d_out.p) (void)hipFree(s->d_out.p);
  for (void* p : extra)
    if (p) (void)hipFree(p);
  if (s->d_desc.p) (void)hipFree(s->d_desc.p);
  if (s->ev0) (void)hipEventDestroy(s->ev0);
  if (s->ev1) (void)hipEventDestroy(s->ev1);
  if (s->stream) (void)hipStreamDestroy(s->stream);
  delete s;
}

// f() with an allocation failure on the host turned into RWKVTTS_ENOMEM.
template <typename F>
static int guard_alloc(const char* who, F&& f) {
  try {
    return f();
  } catch (const std::bad_alloc&) {
    set_error(std::string(who) + ": out of host memory");
    return RWKVTTS_ENOMEM;
  }
}

// A new S on `device` with its stream, its events and its table of n elements on the device: the
// caller's table, or make(T*) when that is null.
template <typename S, typename T, typename Make>
static int stage_create(const char* who, int device, const T* table, size_t n, Make&& make, S** out) {
  S* s = nullptr;
  std::vector<T> own;
  int rc = guard_alloc(who, [&] {
    s = new S();
    if (!table) {
      own.resize(n);
      make(own.data());
      table = own.data();
    }
    return RWKVTTS_OK;
  });
  if (rc) {
    delete s;
    return rc;
  }
  s->device = device;
  auto fail = [&](hipError_t e, const char* what) {
    set_error(std::string(who) + ": " + what + ": " + hipGetErrorString(e));
    stage_free(s);
    return RWKVTTS_EHIP;
  };
  hipError_t e;
  if ((e = hipSetDevice(device)) != hipSuccess) return fail(e, "hipSetDevice");
  if ((e = hipStreamCreate(&s->stream)) != hipSuccess) return fail(e, "hipStreamCreate");
  if ((e = hipEventCreate(&s->ev0)) != hipSuccess) return fail(e, "hipEventCreate");
  if ((e = hipEventCreate(&s->ev1)) != hipSuccess) return fail(e, "hipEventCreate");
  if ((e = hipMalloc(&s->d_table, n * sizeof(T))) != hipSuccess) return fail(e, "hipMalloc");
  if ((e = hipMemcpy(s->d_table, table, n * sizeof(T), hipMemcpyHostToDevice)) != hipSuccess)
    return fail(e, "hipMemcpy");
  *out = s;
  return RWKVTTS_OK;
}

template <typename S>
static int stage_kernel_ms(const char* who, S* s, double* ms) {
  RT_CHECK(s && ms, RWKVTTS_EINVAL, std::string(who) + ": null argument");
  std::lock_guard<std::mutex> lock(s->mu);
  *ms = s->kernel_ms;
  return RWKVTTS_OK;
}

// The three steps of a call around the stage's launches, under s->mu, s->desc built. A window type W
// has in / n_in (host samples), out / out_count (host outputs); windows with out_count == 0 take
// no part. Inputs lie back to back in d_in, outputs back to back in d_out, in the windows' order.
template <typename S>
static int stage_reserve(S* s, int64_t tot_in, int64_t tot_out) {
  RT_HIP(hipSetDevice(s->device));
  int rc;
  if ((rc = s->d_in.reserve((size_t)std::max<int64_t>(tot_in, 1)))) return rc;
  if ((rc = s->d_out.reserve((size_t)tot_out))) return rc;
  return s->d_desc.reserve(s->desc.size());
}

template <typename S, typename W>
static int stage_upload(S* s, const std::vector<W>& ws) {
  int64_t in_off = 0;
  for (const W& w : ws) {
    if (w.out_count == 0) continue;
    if (w.n_in > 0)
      RT_HIP(hipMemcpyAsync(s->d_in.p + in_off, w.in, (size_t)w.n_in * sizeof(float), hipMemcpyHostToDevice, s->stream));
    in_off += w.n_in;
  }
  RT_HIP(hipMemcpyAsync(s->d_desc.p, s->desc.data(), s->desc.size() * sizeof(s->desc[0]), hipMemcpyHostToDevice,
                        s->stream));
  return RWKVTTS_OK;
}

// After the launches: the outputs back, the call's one synchronisation, kernel_ms from the event pair
// (kept as it was if the events cannot be read).
template <typename S, typename W>
static int stage_download(S* s, const std::vector<W>& ws) {
  int64_t out_off = 0;
  for (const W& w : ws) {
    if (w.out_count == 0) continue;
    RT_HIP(hipMemcpyAsync(w.out, s->d_out.p + out_off, (size_t)w.out_count * sizeof(float), hipMemcpyDeviceToHost,
                          s->stream));
    out_off += w.out_count;
  }
  RT_HIP(hipStreamSynchronize(s->stream));
  float ms = 0.0f;
  if (hipEventElapsedTime(&ms, s->ev0, s->ev1) == hipSuccess) s->kernel_ms = (double)ms;
  return RWKVTTS_OK;
}

// The n public structs W at w, n >= 1, whose stride is the caller's struct_size (a later, longer
// struct still reads here): ws[i] = get(element i).
template <typename W, typename E, typename Get>
static int read_windows(const char* who, W* w, int n, std::vector<E>& ws, Get&& get) {
  const size_t stride = w->struct_size;
  RT_CHECK(stride >= sizeof(W), RWKVTTS_EINVAL, std::string(who) + ": struct_size too small");
  ws.resize((size_t)n);
  for (int i = 0; i < n; ++i) {
    W* wi = (W*)((const char*)w + (size_t)i * stride);
    RT_CHECK(wi->struct_size == stride, RWKVTTS_EINVAL, std::string(who) + ": struct_size differs between windows");
    ws[(size_t)i] = get(wi);
  }
  return RWKVTTS_OK;
}

}  // namespace rwkvtts
