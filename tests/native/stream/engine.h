// TEST INFRASTRUCTURE (tests/test_stream_sanitizers.py): a host-only stand-in for csrc/engine.h,
// as tests/native/stub/engine.h is, whose engine also keeps Engine::serve's token-progress contract:
// a job that carries a sink (Job::user, a const rwkvtts_token_sink*) gets its semantic tokens a few
// per "decode step", from the engine's owner thread, in order and each once, and a last call with
// done = 1 before finish(). A request with greedy = 1 is served the old way -- no progress at all,
// the tokens only in the result -- so the manager's completion path has to publish them.
#pragma once
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <string>
#include <thread>
#include <vector>

#include "../../../include/rwkvtts.h"

// ---- the HIP runtime calls manager.cpp makes (host memory) ----
typedef int hipError_t;
typedef void* hipStream_t;
constexpr hipError_t hipSuccess = 0;
enum { hipMemcpyHostToDevice = 1, hipStreamNonBlocking = 1 };
inline const char* hipGetErrorString(hipError_t) { return "stub"; }
inline hipError_t hipGetDevice(int* d) { *d = 0; return hipSuccess; }
inline hipError_t hipSetDevice(int) { return hipSuccess; }
inline hipError_t hipMalloc(void** p, size_t n) { *p = malloc(n ? n : 1); return *p ? hipSuccess : 2; }
inline hipError_t hipFree(void* p) { free(p); return hipSuccess; }
inline hipError_t hipMemcpy(void* d, const void* s, size_t n, int) { memcpy(d, s, n); return hipSuccess; }
inline hipError_t hipMemcpyPeer(void* d, int, const void* s, int, size_t n) { memcpy(d, s, n); return hipSuccess; }
inline hipError_t hipStreamCreateWithFlags(hipStream_t* s, unsigned) { *s = nullptr; return hipSuccess; }
inline hipError_t hipStreamSynchronize(hipStream_t) { return hipSuccess; }
inline hipError_t hipStreamDestroy(hipStream_t) { return hipSuccess; }

namespace rwkvtts {
void set_error(const std::string& msg);
#define RT_HIP(expr)                                          \
  do {                                                       \
    hipError_t _e = (expr);                                  \
    if (_e != hipSuccess) {                                  \
      ::rwkvtts::set_error(std::string(#expr) + ": stub");   \
      return RWKVTTS_EHIP;                                   \
    }                                                        \
  } while (0)
#define RT_CHECK(cond, code, msg) \
  do {                            \
    if (!(cond)) {                \
      ::rwkvtts::set_error(msg);  \
      return code;                \
    }                             \
  } while (0)

struct Job {
  rwkvtts_request req{};
  rwkvtts_result* res = nullptr;
  void* user = nullptr;
};
class Engine;
class JobSource {
 public:
  virtual ~JobSource() = default;
  virtual bool next(int max, bool wait, std::vector<Job*>& out) = 0;
  virtual void finish(Job* j) = 0;
  virtual void progress(const Engine&) {}
};

// the stub's tokens: a function of the seed (manager_stream_tsan_main.cpp checks them)
inline int32_t stub_semantic(uint64_t seed, int i) { return (int32_t)((seed * 7 + (uint64_t)i) % 8192); }
inline int32_t stub_global(uint64_t seed, int g) { return (int32_t)((seed + (uint64_t)g) % 4096); }

// STUB_FAIL_SEED (env, read at init): the request with this seed fails with RWKVTTS_EHIP after half
// of its tokens went out (the unit that would have brought the next ones faulted).
class Engine {
 public:
  int init(const rwkvtts_engine_desc& desc, const void* w, size_t bytes, int) {
    RT_CHECK(w && bytes > 0, RWKVTTS_EINVAL, "stub: no weights");
    device_ = desc.device;
    S_ = desc.max_slots > 0 ? desc.max_slots : 4;
    if (const char* e = getenv("STUB_FAIL_SEED")) fail_seed_ = atoll(e);
    return RWKVTTS_OK;
  }
  bool persistent() const { return device_ == 0; }
  bool take_recovered() { return false; }
  int serve(JobSource& src) {
    struct A {
      Job* j;
      int made;                  // tokens generated so far
      std::vector<int32_t> sem;  // (the engine's own buffer: the sink's pointers are valid during the call only)
    };
    std::vector<A> act;
    bool open = true;
    while (true) {
      if (open && (int)act.size() < S_) {
        std::vector<Job*> fresh;
        open = src.next(S_ - (int)act.size(), act.empty(), fresh);
        for (Job* j : fresh) act.push_back({j, 0, {}});
      }
      if (act.empty()) {
        if (!open) return RWKVTTS_OK;
        continue;
      }
      std::this_thread::sleep_for(std::chrono::microseconds(200));  // one "unit of work"
      stats.steps++;
      max_active = std::max<int64_t>(max_active, (int64_t)act.size());
      for (size_t i = 0; i < act.size();) {
        A& a = act[i];
        Job* j = a.j;
        rwkvtts_result& r = *j->res;
        const uint64_t seed = j->req.seed;
        const int total = j->req.fixed_semantic;
        const rwkvtts_token_sink* sink = j->req.greedy ? nullptr : (const rwkvtts_token_sink*)j->user;
        int32_t glob[RWKVTTS_N_GLOBAL];
        for (int g = 0; g < RWKVTTS_N_GLOBAL; ++g) glob[g] = stub_global(seed, g);
        if (fail_seed_ >= 0 && seed == (uint64_t)fail_seed_ && a.made >= total / 2) {
          r.status = RWKVTTS_EHIP;
          r.n_global = r.n_semantic = 0;
          if (sink && sink->fn) sink->fn(sink->user, nullptr, 0, nullptr, a.made, 0, 1, r.status);
          src.finish(j);
          act.erase(act.begin() + i);
          continue;
        }
        const int first = a.made, count = std::min(total - first, 1 + (int)(seed % 3));
        for (int k = 0; k < count; ++k) a.sem.push_back(stub_semantic(seed, first + k));
        a.made += count;
        const bool done = a.made >= total;
        if (sink && sink->fn) sink->fn(sink->user, glob, RWKVTTS_N_GLOBAL, a.sem.data() + first, first, count, done ? 1 : 0, 0);
        if (!done) {
          ++i;
          continue;
        }
        r.status = 0;
        r.n_global = RWKVTTS_N_GLOBAL;
        memcpy(r.global_tokens, glob, sizeof(glob));
        r.n_semantic = total;
        if (total > 0) memcpy(r.semantic_tokens, a.sem.data(), sizeof(int32_t) * total);
        src.finish(j);
        act.erase(act.begin() + i);
      }
      src.progress(*this);
    }
  }
  rwkvtts_stats stats{};
  int64_t max_active = 0;

 private:
  int device_ = 0, S_ = 4;
  long long fail_seed_ = -1;
};
}  // namespace rwkvtts
