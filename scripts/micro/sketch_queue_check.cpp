// sketch_queue_check.cpp -- the scheduling of the sketch pipeline (wfmash_amd/host/sketch_queue.hpp) without a device, for the
// sanitizers:
//
//   g++ -std=c++17 -O1 -g -fsanitize=thread -pthread scripts/micro/sketch_queue_check.cpp -o sketch_queue_tsan && ./sketch_queue_tsan
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -pthread scripts/micro/sketch_queue_check.cpp -o sketch_queue_asan && ./sketch_queue_asan
//
// As in minmers.cpp's SketchRun: a feeder admits items of random lengths into the window and routes each to the "device" stage,
// to the streamer (one ring slot per chunk, then the workers) or straight to the workers; the device stage hands every third
// item back to the streamer, finishes one in three itself and leaves the closing of the rest to a worker; whoever makes an
// item final retires it; the feeder delivers in input order.  Checked: delivery 0, 1, 2, ... exactly once, every slot back,
// the window at zero, every thread joined.  Then each configuration with a stage that fails at a fixed item (device,
// streamer, worker): the call returns, the error is the first one set, delivery stays in order.  Then with an exception
// thrown in the feeder, between two items and with an item admitted but not yet queued: once left to the joiner, which must
// bring everything down, and once caught as add_minmers_core catches it, where the drain must still end (an item is listed
// only once a stage has it).  Exit status 0 = all held.
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <stdexcept>
#include <thread>
#include <vector>

#include "../../wfmash_amd/host/sketch_queue.hpp"

namespace {

enum Route { kDevice = 0, kStream = 1, kDirect = 2 };
enum Fail { kNoFail = 0, kFailDevice, kFailStreamer, kFailWorker };

struct Item {
  int64_t idx = 0, len = 0;
  int route = kDirect, chunks = 1;
  std::atomic<int> pending{0};
  bool closing_only = false;  // "winnowed on the device": a worker only closes it
};
struct Task { Item* item; int chunk; int slot; };

// throw_at >= 0: the feeder throws there -- throw_where 0: between two items; 1: with the item admitted and in its hands, not yet queued.
// caught: the feeder's caller catches, closes, drains and joins as add_minmers_core does; otherwise the joiner's destructor is all there is.
struct Config { int workers, dev_threads, nslots; int64_t window_max; int items; Fail fail; int64_t fail_at; int64_t throw_at; int throw_where; bool caught; };

std::atomic<int> g_alive{0};  // threads of the stages that are running
struct Alive { Alive() { ++g_alive; } ~Alive() { --g_alive; } };

struct Run {
  const Config& C;
  std::vector<std::unique_ptr<Item>> items;
  std::vector<std::atomic<int64_t>> ring;  // who holds the slot (-1: nobody)
  std::vector<int64_t>& delivered;
  std::atomic<bool> bad{false}, fired{false};
  skch::Handoff<Task> work;
  skch::Handoff<Item*> to_stream, to_device;
  skch::SlotPool slots;
  skch::InflightWindow window;
  skch::DeliveryCursor cursor;
  skch::FirstError err;
  skch::StageThreads<Task, Item*> threads{work, to_stream, to_device};

  Run(const Config& c, std::vector<int64_t>& out)
      : C(c), items((size_t)c.items), ring((size_t)c.nslots), delivered(out), slots(c.nslots), window(c.window_max), cursor(c.items) {
    for (auto& r : ring) r.store(-1);
  }
  void fail_here(Fail kind, const Item* it) {
    if (C.fail != kind || it->idx < C.fail_at || fired.exchange(true)) return;  // the first item from fail_at on that comes by
    err.set(-7, "the first error");
    err.set(-9, "a later error");
  }
  void retire(Item* it) {
    cursor.mark_final(it->idx);
    window.retire(it->len);
  }
  void worker_loop() {
    Alive a;
    for (Task t; work.pop(&t);) {
      Item* it = t.item;
      if (it->closing_only) { fail_here(kFailWorker, it); retire(it); continue; }
      if (t.slot >= 0) {
        if (ring[(size_t)t.slot].exchange(-1) != it->idx) bad.store(true);  // the slot is ours until we give it back
        slots.give(t.slot);
      }
      if ((it->idx + t.chunk) % 5 == 0) std::this_thread::sleep_for(std::chrono::microseconds(100));  // finish out of order
      if (it->pending.fetch_sub(1) == 1) { fail_here(kFailWorker, it); retire(it); }
    }
  }
  void streamer_loop() {
    Alive a;
    for (Item* it; to_stream.pop(&it);) {
      fail_here(kFailStreamer, it);
      for (int c = 0; c < it->chunks; ++c) {
        const int slot = slots.take();
        if (ring[(size_t)slot].exchange(it->idx) != -1) bad.store(true);  // handed out twice
        work.push(Task{it, c, slot});
      }
    }
  }
  void device_loop(int) {
    Alive a;
    for (Item* it; to_device.pop(&it);) {
      fail_here(kFailDevice, it);
      if (it->idx % 7 == 0) std::this_thread::sleep_for(std::chrono::microseconds(150));
      switch ((it->idx / 3) % 3) {
        case 0: to_stream.push(it); break;  // handed back
        case 1: retire(it); break;          // finished on the device
        default: it->closing_only = true; work.push(Task{it, 0, -1});
      }
    }
  }
  void deliver_ready(int64_t limit) {
    for (int64_t i; (i = cursor.take(limit)) >= 0;) delivered.push_back(i);
  }
  void feed_one(int64_t i, std::mt19937& rng) {
    if (C.throw_where == 0 && i == C.throw_at) throw std::runtime_error("the feeder fails between two items");
    auto it = std::make_unique<Item>();
    it->idx = i;
    it->len = 1 + (int64_t)(rng() % 5000);
    it->route = (int)(rng() % 3);
    it->chunks = it->route == kDirect ? 1 : 1 + (int)(rng() % 4);
    it->pending.store(it->chunks);
    if (it->len % 11 == 0) { cursor.mark_final(i); return; }  // "shorter than k": no job
    window.admit(it->len);
    deliver_ready(i);
    if (C.throw_where == 1 && C.throw_at >= 0 && i >= C.throw_at) {  // admitted and in the feeder's hands, not yet queued
      window.retire(it->len);
      throw std::runtime_error("the feeder fails with an item in its hands");
    }
    Item* p = it.get();
    if (p->route == kDevice) to_device.push(p);
    else if (p->route == kStream) to_stream.push(p);
    else work.push(Task{p, 0, -1});
    items[(size_t)i] = std::move(it);  // in items[] only once a stage has it: what is there will be made final
  }
  void start_and_feed() {
    threads.start_workers(C.workers, [this] { worker_loop(); });
    threads.start_device(C.dev_threads, [this](int t) { device_loop(t); });
    threads.start_streamer([this] { streamer_loop(); });
    std::mt19937 rng(12345u + (unsigned)C.items);
    for (int64_t i = 0; i < C.items; ++i) feed_one(i, rng);
  }
  // as add_minmers_core ends, after an exception in the feeder too: what never got a job counts as final
  void close_drain_join() {
    threads.close_feed();
    for (int64_t i = 0; i < C.items; ++i)
      if (!items[(size_t)i]) cursor.mark_final(i);
    while (!cursor.done()) { cursor.wait_next(window); deliver_ready(C.items); }
    threads.join();
  }
};

bool in_order(const std::vector<int64_t>& d) {
  for (size_t i = 0; i < d.size(); ++i)
    if (d[i] != (int64_t)i) return false;
  return true;
}

// -> items delivered, or -1 if something did not hold
long run(const Config& C) {
  std::vector<int64_t> delivered;
  bool threw = false;
  {
    Run R(C, delivered);
    try {
      R.start_and_feed();
    } catch (const std::runtime_error&) {
      threw = true;
    }
    if (!threw || C.caught) {
      R.close_drain_join();
      if (!R.threads.all_joined() || R.slots.free_slots() != (size_t)C.nslots || R.window.inflight() != 0) return -1;
      if (C.fail == kNoFail ? R.err.code() != 0 : (R.err.code() != -7 || !R.err.text() || strcmp(R.err.text(), "the first error") != 0)) return -1;
      if (R.bad.load()) return -1;
    }
  }  // (an exception nobody handles: R's joiner alone closes the hand-offs and joins)
  if (g_alive.load() != 0 || !in_order(delivered)) return -1;
  if (threw != (C.throw_at >= 0)) return -1;
  if ((!threw || C.caught) && (long)delivered.size() != C.items) return -1;
  if (threw && !C.caught && (long)delivered.size() > C.throw_at) return -1;
  return (long)delivered.size();
}

}  // namespace

int main() {
  long total = 0;
  const int n = 3000;
  for (int workers : {1, 2, 8}) {
    for (int dev : {1, 2, 4}) {
      const int nslots = workers == 1 ? 1 : 16;                                // one ring has a single slot
      const int64_t wmax = dev == 2 ? 1000 : (workers == 8 ? 20000 : 1 << 30);  // one window is smaller than the largest item (5000)
      const long ok = run(Config{workers, dev, nslots, wmax, n, kNoFail, -1, -1, 0, false});
      if (ok != n) { fprintf(stderr, "FAILED: %d workers, %d device threads: %ld\n", workers, dev, ok); return 1; }
      total += ok;
      for (Fail f : {kFailDevice, kFailStreamer, kFailWorker}) {
        const long m = run(Config{workers, dev, nslots, wmax, n, f, 1200, -1, 0, false});  // the first item from 1200 on that reaches stage f
        if (m != n) { fprintf(stderr, "FAILED with a failing stage %d: %d workers, %d device threads: %ld\n", (int)f, workers, dev, m); return 1; }
        total += m;
      }
      printf("%d workers x %d device threads, %d slots, window %lld: %d items in order; the same with a failing device stage, streamer, worker: first error kept, all joined\n",
             workers, dev, nslots, (long long)wmax, n);
    }
  }
  for (int where : {0, 1}) {
    for (bool caught : {false, true}) {
      const long t = run(Config{8, 2, 16, 20000, n, kNoFail, -1, 1700, where, caught});
      if (t < 0) { fprintf(stderr, "FAILED with an exception in the feeder at item 1700 (where %d, caught %d)\n", where, (int)caught); return 1; }
      total += t;
      printf("an exception in the feeder at item 1700 (%s; %s): %ld delivered in order, all joined\n", where ? "an item in its hands" : "between two items",
             caught ? "caught: closed, drained, joined" : "not caught: the joiner alone", t);
    }
  }
  printf("sketch_queue_check: ok, %ld items passed through\n", total);
  return 0;
}
