// map_queue.hpp -- the two hand-offs of the map driver (mapper.cpp), over any payload type: no device type in here, so
// scripts/micro/map_queue_check.cpp drives them under the thread sanitizer.
#pragma once

#include <atomic>
#include <condition_variable>
#include <cstdint>
#include <deque>
#include <map>
#include <memory>
#include <mutex>
#include <thread>
#include <utility>
#include <vector>

namespace skch {

// Takes (seq, payload) from any thread and hands the payloads to the sink in seq order, 0 upwards, under its lock: what came early
// waits.  Sink: write(Payload&) per payload, flush() once at the end of every put, whether it wrote or not.
template <class Payload, class Sink>
class OrderedWriter {
 public:
  explicit OrderedWriter(Sink sink) : sink_(std::move(sink)) {}
  void put(uint64_t seq, Payload&& p) {
    std::lock_guard<std::mutex> lk(mu_);
    pending_.emplace(seq, std::move(p));
    for (auto it = pending_.begin(); it != pending_.end() && it->first == next_; it = pending_.erase(it), ++next_) sink_.write(it->second);
    sink_.flush();
  }

 private:
  std::mutex mu_;
  std::map<uint64_t, Payload> pending_;
  uint64_t next_ = 0;
  Sink sink_;
};

// The bounded hand-off from one producer (a device thread) to its consumer threads.
//  * one item may wait: with the one in the producer's hands and one per consumer that bounds what is alive;
//  * consumers are started by the producer, one at a time (start_one), so a call of one batch starts one;
//  * push() waits for room, or returns at once when `error` is set -- the item still goes in and is dropped by whoever pops it,
//    or with the queue;
//  * a consumer that ends, for whatever reason, wakes the producer, which then sees the error that ended it;
//  * the destructor closes the queue and joins every consumer: declare it after what the consumers use.
template <class Item>
class StageQueue {
 public:
  explicit StageQueue(const std::atomic<int>& error) : error_(error) {}
  StageQueue(const StageQueue&) = delete;
  StageQueue& operator=(const StageQueue&) = delete;
  ~StageQueue() {
    { std::lock_guard<std::mutex> lk(mu_); closed_ = true; }
    cv_.notify_all();
    for (auto& t : threads_) if (t.joinable()) t.join();
  }
  size_t consumers() const { return threads_.size(); }
  // producer only.  entry(): the consumer's thread function, a loop over pop()
  template <class Entry>
  void start_one(Entry entry) {
    threads_.emplace_back([this, entry] {
      entry();
      { std::lock_guard<std::mutex> lk(mu_); }  // (the producer is either before its look at the error or already waiting: no wake-up is lost)
      cv_.notify_all();
    });
  }
  void push(std::unique_ptr<Item> item) {
    {
      std::unique_lock<std::mutex> lk(mu_);
      cv_.wait(lk, [&] { return queue_.size() < 1 || error_.load() != 0; });
      queue_.push_back(std::move(item));
    }
    cv_.notify_all();
  }
  // the next item, or null once the queue is closed and empty
  std::unique_ptr<Item> pop() {
    std::unique_ptr<Item> item;
    {
      std::unique_lock<std::mutex> lk(mu_);
      cv_.wait(lk, [&] { return !queue_.empty() || closed_; });
      if (queue_.empty()) return nullptr;
      item = std::move(queue_.front());
      queue_.pop_front();
    }
    cv_.notify_all();
    return item;
  }

 private:
  const std::atomic<int>& error_;
  std::mutex mu_;
  std::condition_variable cv_;
  std::deque<std::unique_ptr<Item>> queue_;
  bool closed_ = false;
  std::vector<std::thread> threads_;
};

}  // namespace skch
