// map_queue_check.cpp -- the map driver's two hand-offs (wfmash_amd/host/map_queue.hpp) without a device, for the sanitizers:
//
//   g++ -std=c++17 -O1 -g -fsanitize=thread -pthread scripts/micro/map_queue_check.cpp -o map_queue_tsan && ./map_queue_tsan
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -pthread scripts/micro/map_queue_check.cpp -o map_queue_asan && ./map_queue_asan
//
// As in the driver: several producers ("device threads") take numbered items from one counter, each hands them to a StageQueue of
// its own with 1, 2 or 4 consumers ("filter threads"), started one per item; the consumers pass them to one OrderedWriter, whose sink
// must see 0, 1, 2, ... .  Then the same with a consumer that fails in mid-stream: the error is set, its thread ends, the producers
// must come back from push() and every thread must be joined.  Prints the number of items that passed; exit status 0 = all held.
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <mutex>
#include <thread>
#include <vector>

#include "../../wfmash_amd/host/map_queue.hpp"

namespace {

struct Item { uint64_t seq; std::vector<int> body; };
struct Out { uint64_t seq; long sum; };

struct Sink {
  std::vector<uint64_t>* seen;
  long* flushes;
  void write(Out& o) { seen->push_back(o.seq); }
  void flush() { ++*flushes; }
};

// -> items that reached the sink, or -1 if they came out of order; fail_at < 0: no failure
long run(int producers, size_t consumers, uint64_t items, long fail_at) {
  std::atomic<int> error{0};
  std::atomic<uint64_t> next{0};
  std::vector<uint64_t> seen;
  long flushes = 0;
  skch::OrderedWriter<Out, Sink> writer(Sink{&seen, &flushes});
  auto producer = [&](int p) {
    skch::StageQueue<Item> queue(error);
    auto consumer = [&] {
      for (;;) {
        std::unique_ptr<Item> it = queue.pop();
        if (!it) return;
        if (error.load() != 0) continue;  // after an error items are only taken out
        if ((long)it->seq == fail_at) { error.store(-7); return; }  // as a filter thread that threw: error set, thread over
        long sum = 0;
        for (int v : it->body) sum += v;
        if ((it->seq + (uint64_t)p) % 3 == 0) std::this_thread::sleep_for(std::chrono::microseconds(200));  // finish out of order
        writer.put(it->seq, Out{it->seq, sum});
      }
    };
    for (;;) {
      if (error.load() != 0) break;
      const uint64_t seq = next.fetch_add(1);
      if (seq >= items) break;
      std::unique_ptr<Item> it(new Item{seq, std::vector<int>(16 + seq % 5, (int)seq)});
      if (queue.consumers() < consumers) queue.start_one(consumer);
      queue.push(std::move(it));
    }
  };  // (the queue's destructor closes it and joins the consumers)
  std::vector<std::thread> pool;
  for (int p = 1; p < producers; ++p) pool.emplace_back(producer, p);
  producer(0);
  for (auto& t : pool) t.join();
  for (size_t i = 0; i < seen.size(); ++i)
    if (seen[i] != i) return -1;
  if (flushes < (long)seen.size()) return -1;
  if (fail_at < 0 && (seen.size() != items || error.load() != 0)) return -1;
  if (fail_at >= 0 && (error.load() != -7 || (long)seen.size() > fail_at)) return -1;  // nothing at or after the failed item can be written
  return (long)seen.size();
}

}  // namespace

int main() {
  long total = 0;
  for (size_t consumers : {1, 2, 4}) {
    for (int producers : {1, 3}) {
      const long n = run(producers, consumers, 2000, -1);
      if (n != 2000) { fprintf(stderr, "FAILED: %d producers, %zu consumers: %ld\n", producers, consumers, n); return 1; }
      total += n;
      const long m = run(producers, consumers, 2000, 700);
      if (m < 0) { fprintf(stderr, "FAILED with an error at item 700: %d producers, %zu consumers\n", producers, consumers); return 1; }
      total += m;
      printf("%d producers x %zu consumers: 2000 items in order; with a failure at item 700: %ld written, all joined\n", producers, consumers, m);
    }
  }
  printf("map_queue_check: ok, %ld items passed through\n", total);
  return 0;
}
