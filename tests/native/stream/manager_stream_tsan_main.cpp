// TEST INFRASTRUCTURE (tests/test_stream_sanitizers.py): csrc/manager.cpp's streaming entry points
// (rwkvtts_manager_submit_stream / _wait_tokens beside submit / wait) driven from many threads under
// ThreadSanitizer, against the stub engine of stream/engine.h, which delivers partial tokens from the
// engine's owner thread.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <atomic>
#include <chrono>
#include <string>
#include <thread>
#include <vector>

#include "engine.h"

namespace rwkvtts {
static thread_local std::string g_err;
void set_error(const std::string& m) { g_err = m; }
}  // namespace rwkvtts
extern "C" const char* rwkvtts_last_error(void) { return rwkvtts::g_err.c_str(); }
using rwkvtts::stub_global;
using rwkvtts::stub_semantic;

static std::atomic<int> fails{0};
#define EXPECT(c)                                                            \
  do {                                                                       \
    if (!(c)) {                                                              \
      fprintf(stderr, "expectation failed at line %d: %s\n", __LINE__, #c); \
      ++fails;                                                               \
    }                                                                        \
  } while (0)

static rwkvtts_manager* make(int n_engines, int slots, int collect_ms) {
  rwkvtts_manager_desc d;
  memset(&d, 0, sizeof(d));
  d.n_engines = n_engines;
  for (int i = 0; i < n_engines; ++i) d.devices[i] = i;
  d.engine.max_slots = slots;
  d.max_batch_size = 8;
  d.collect_timeout_ms = collect_ms;
  static char w[4096];
  rwkvtts_manager* m = nullptr;
  EXPECT(rwkvtts_manager_create(&d, w, sizeof(w), &m) == RWKVTTS_OK);
  return m;
}

static rwkvtts_request req(uint64_t seed, int fixed, int silent) {
  static const int32_t text[4] = {12300, 12301, 12302, 12303};
  rwkvtts_request q;
  memset(&q, 0, sizeof(q));
  q.text_tokens = text;
  q.n_text = 4;
  q.has_seed = 1;
  q.seed = seed;
  q.max_tokens = 64;
  q.fixed_semantic = fixed;
  q.greedy = silent;  // stream/engine.h: 1 = the old engine behaviour, no progress for this request
  return q;
}

struct Seen {
  int polls = 0, partial = 0;  // wait_tokens calls that returned; those with 0 < n < total and !done
  int status = 0, n = 0;
};

// polls one ticket to its end: every answer is a growing prefix of the stub's tokens
// (may_vanish: another thread's wait() may release the ticket between two polls -> status 1)
static Seen follow(rwkvtts_manager* m, uint64_t ticket, uint64_t seed, int total, int timeout_ms,
                   bool may_vanish = false) {
  Seen s;
  std::vector<int32_t> sem(RWKVTTS_SEMANTIC_LIMIT);
  int32_t glob[RWKVTTS_N_GLOBAL];
  int have = 0;
  while (true) {
    int32_t ng = -1, ns = -1, done = -1, status = -1;
    const int rc = rwkvtts_manager_wait_tokens(m, ticket, have, timeout_ms, glob, &ng, sem.data(), &ns, &done, &status);
    if (may_vanish && rc == RWKVTTS_EINVAL) {
      s.status = 1;
      s.n = have;
      break;
    }
    EXPECT(rc == RWKVTTS_OK || rc == RWKVTTS_EBUSY);
    if (rc != RWKVTTS_OK && rc != RWKVTTS_EBUSY) break;
    EXPECT(ns >= have && ns <= total);                  // never shrinks
    EXPECT(rc == RWKVTTS_EBUSY || ns > have || done);   // OK means news
    for (int i = 0; i < ns; ++i) EXPECT(sem[i] == stub_semantic(seed, i));
    if (ng > 0) {
      EXPECT(ng == RWKVTTS_N_GLOBAL);
      for (int g = 0; g < ng; ++g) EXPECT(glob[g] == stub_global(seed, g));
    }
    if (ns > 0) EXPECT(ng == RWKVTTS_N_GLOBAL);         // semantic tokens never come before the speaker
    ++s.polls;
    if (!done && ns > 0 && ns < total) ++s.partial;
    have = ns;
    if (done) {
      s.status = status;
      s.n = ns;
      break;
    }
  }
  return s;
}

static void check_final(rwkvtts_manager* m, uint64_t ticket, uint64_t seed, int total, const Seen& s) {
  std::vector<int32_t> sem(RWKVTTS_SEMANTIC_LIMIT);
  rwkvtts_result r;
  memset(&r, 0, sizeof(r));
  r.semantic_tokens = sem.data();
  EXPECT(rwkvtts_manager_wait(m, ticket, -1, &r) == RWKVTTS_OK);
  EXPECT(r.status == s.status);
  if (r.status == 0) {
    EXPECT(r.n_semantic == total && s.n == total);      // the stream ended with every token
    for (int i = 0; i < total; ++i) EXPECT(sem[i] == stub_semantic(seed, i));
  }
  // the ticket is released now
  int32_t ns = 0, done = 0;
  EXPECT(rwkvtts_manager_wait_tokens(m, ticket, 0, 0, nullptr, nullptr, nullptr, &ns, &done, nullptr) == RWKVTTS_EINVAL);
}

// streamed, silently-served and plain requests from many threads at once over two engines
static void scenario_concurrent() {
  rwkvtts_manager* m = make(2, 4, 1);
  std::atomic<int> partial{0}, polls{0};
  std::vector<std::thread> th;
  for (int t = 0; t < 6; ++t)
    th.emplace_back([&, t] {
      for (int i = 0; i < 10; ++i) {
        const uint64_t seed = 100 * t + i;
        const int total = 50 + 3 * i, kind = (t + i) % 3;  // 0 streamed, 1 streamed on a silent engine, 2 plain submit
        rwkvtts_request q = req(seed, total, kind == 1);
        uint64_t id = 0;
        if (kind == 2) EXPECT(rwkvtts_manager_submit(m, &q, &id) == RWKVTTS_OK);
        else EXPECT(rwkvtts_manager_submit_stream(m, &q, &id) == RWKVTTS_OK);
        const Seen s = follow(m, id, seed, total, i % 2 ? -1 : 1);
        EXPECT(s.status == 0 && s.n == total);
        if (kind != 0) EXPECT(s.partial == 0);  // no progress: everything arrives with completion
        else partial += s.partial;
        polls += s.polls;
        check_final(m, id, seed, total, s);
      }
    });
  for (auto& x : th) x.join();
  EXPECT(partial > 0);  // some streamed request was seen mid-way
  rwkvtts_manager_stats st;
  EXPECT(rwkvtts_manager_get_stats(m, &st) == RWKVTTS_OK && st.completed == 60 && st.waiters == 0);
  EXPECT(rwkvtts_manager_destroy(m) == RWKVTTS_OK);
}

// one thread polls a ticket while another waits for its result: the second is refused while the
// first is blocked, and both kinds of call work one after the other
static void scenario_poll_then_wait() {
  rwkvtts_manager* m = make(1, 2, 1);
  rwkvtts_request q = req(7, 400, 0);
  uint64_t id = 0;
  EXPECT(rwkvtts_manager_submit_stream(m, &q, &id) == RWKVTTS_OK);
  std::thread poller([&] {
    const Seen s = follow(m, id, 7, 400, -1, true);
    EXPECT(s.status == 1 || (s.status == 0 && s.n == 400));
  });
  std::vector<int32_t> sem(RWKVTTS_SEMANTIC_LIMIT);
  rwkvtts_result r;
  memset(&r, 0, sizeof(r));
  r.semantic_tokens = sem.data();
  int rc;  // refused (EINVAL) whenever the poller holds the ticket, busy or ready otherwise
  while ((rc = rwkvtts_manager_wait(m, id, 0, &r)) != RWKVTTS_OK) EXPECT(rc == RWKVTTS_EINVAL || rc == RWKVTTS_EBUSY);
  EXPECT(r.status == 0 && r.n_semantic == 400 && sem[399] == stub_semantic(7, 399));
  poller.join();  // (its last call may find the ticket released: follow() stops there)
  EXPECT(rwkvtts_manager_destroy(m) == RWKVTTS_OK);
}

// a request that fails half-way: the stream ends with done and the status, what was delivered stands
static void scenario_failure() {
  setenv("STUB_FAIL_SEED", "31", 1);
  rwkvtts_manager* m = make(1, 2, 1);
  unsetenv("STUB_FAIL_SEED");
  uint64_t bad = 0, good = 0;
  rwkvtts_request qb = req(31, 40, 0), qg = req(32, 40, 0);
  EXPECT(rwkvtts_manager_submit_stream(m, &qb, &bad) == RWKVTTS_OK);
  EXPECT(rwkvtts_manager_submit_stream(m, &qg, &good) == RWKVTTS_OK);
  const Seen sb = follow(m, bad, 31, 40, -1), sg = follow(m, good, 32, 40, -1);
  EXPECT(sb.status == RWKVTTS_EHIP && sb.n >= 20 && sb.n < 40);
  EXPECT(sg.status == 0 && sg.n == 40);
  check_final(m, bad, 31, 40, sb);
  check_final(m, good, 32, 40, sg);
  EXPECT(rwkvtts_manager_destroy(m) == RWKVTTS_OK);
}

// destroy while wait_tokens callers are blocked and requests are still queued: every caller returns
static void scenario_destroy_with_pollers() {
  rwkvtts_manager* m = make(2, 2, 1);
  std::vector<uint64_t> tk(40);
  for (int i = 0; i < 40; ++i) {
    rwkvtts_request q = req(i, 30, i % 2);
    EXPECT(rwkvtts_manager_submit_stream(m, &q, &tk[i]) == RWKVTTS_OK);
  }
  std::atomic<int> returned{0}, started{0};
  std::vector<std::thread> th;
  for (int t = 0; t < 4; ++t)
    th.emplace_back([&, t] {
      std::vector<int32_t> sem(RWKVTTS_SEMANTIC_LIMIT);
      int32_t ns = 0, done = 0, status = 0;
      ++started;
      // (have = the limit: only completion or the shutdown can wake this caller)
      const int rc = rwkvtts_manager_wait_tokens(m, tk[39 - t], RWKVTTS_SEMANTIC_LIMIT, -1, nullptr, nullptr, sem.data(),
                                                 &ns, &done, &status);
      EXPECT(rc == RWKVTTS_OK || rc == RWKVTTS_ECLOSED);
      if (rc == RWKVTTS_OK) EXPECT(done == 1 && status == 0 && ns == 30);
      ++returned;
    });
  while (started < 4) std::this_thread::yield();
  std::this_thread::sleep_for(std::chrono::milliseconds(2));
  EXPECT(rwkvtts_manager_destroy(m) == RWKVTTS_OK);
  for (auto& x : th) x.join();
  EXPECT(returned == 4);
}

int main() {
  scenario_concurrent();
  scenario_poll_then_wait();
  scenario_failure();
  scenario_destroy_with_pollers();
  if (fails) {
    fprintf(stderr, "%d expectations failed\n", fails.load());
    return 1;
  }
  printf("manager_stream_tsan: ok\n");
  return 0;
}
