// sketch_queue.hpp -- the scheduling of the sketch pipeline (minmers.cpp, SketchRun), over any payload type: no device type in
// here, so scripts/micro/sketch_queue_check.cpp drives it with fake stages under the thread sanitizer.
//
// The pipeline: a feeder (the calling thread) routes every item to the device stage, to the streamer (which takes a slot of
// the ring per chunk and passes it to the workers) or straight to the workers.  The device stage may hand an item back to
// the streamer, finish it, or leave its closing to a worker.  Whoever makes an item final retires it from the window; the
// calling thread hands final items on in input order.
#pragma once

#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <cstdint>
#include <deque>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <utility>
#include <vector>

namespace skch {

// A closable hand-off, any number of producers and consumers.  pop() returns false once it is closed and empty.
template <class T>
class Handoff {
 public:
  void push(T item) {
    { std::lock_guard<std::mutex> lk(mu_); items_.push_back(std::move(item)); }
    cv_.notify_one();
  }
  bool pop(T* item) {
    std::unique_lock<std::mutex> lk(mu_);
    cv_.wait(lk, [&] { return closed_ || !items_.empty(); });
    if (items_.empty()) return false;
    *item = std::move(items_.front());
    items_.pop_front();
    return true;
  }
  void close() {
    { std::lock_guard<std::mutex> lk(mu_); closed_ = true; }
    cv_.notify_all();
  }

 private:
  std::mutex mu_;
  std::condition_variable cv_;
  std::deque<T> items_;
  bool closed_ = false;
};

// The free slots of a ring: take() waits for one.
class SlotPool {
 public:
  explicit SlotPool(int n) { for (int i = 0; i < n; ++i) free_.push_back(i); }
  int take() {
    std::unique_lock<std::mutex> lk(mu_);
    cv_.wait(lk, [&] { return !free_.empty(); });
    const int slot = free_.back();
    free_.pop_back();
    return slot;
  }
  void give(int slot) {
    { std::lock_guard<std::mutex> lk(mu_); free_.push_back(slot); }
    cv_.notify_one();
  }
  size_t free_slots() { std::lock_guard<std::mutex> lk(mu_); return free_.size(); }

 private:
  std::mutex mu_;
  std::condition_variable cv_;
  std::vector<int> free_;
};

// What is in work, by size.  An item larger than the window goes in alone (the `inflight == 0` clause).
class InflightWindow {
 public:
  explicit InflightWindow(int64_t max) : max_(max) {}
  void admit(int64_t len) {
    std::unique_lock<std::mutex> lk(mu_);
    cv_.wait(lk, [&] { return inflight_ == 0 || inflight_ + len <= max_; });
    inflight_ += len;
  }
  // wakes the feeder (admit) and the in-order drain (wait_for)
  void retire(int64_t len) {
    { std::lock_guard<std::mutex> lk(mu_); inflight_ -= len; }
    cv_.notify_all();
  }
  // waits until `settled` holds; it is looked at after every retire()
  template <class Pred>
  void wait_for(Pred settled) {
    std::unique_lock<std::mutex> lk(mu_);
    cv_.wait(lk, settled);
  }
  int64_t inflight() { std::lock_guard<std::mutex> lk(mu_); return inflight_; }

 private:
  const int64_t max_;
  std::mutex mu_;
  std::condition_variable cv_;
  int64_t inflight_ = 0;
};

// In-order delivery: item i is handed on only when every item before it is final, while later ones are still in work.
// mark_final(i) from any thread, BEFORE the item is retired from the window (wait_next sleeps on the window); take() and
// wait_next() from the one delivering thread.
class DeliveryCursor {
 public:
  explicit DeliveryCursor(int64_t n) : n_(n), final_(new std::atomic<bool>[(size_t)std::max<int64_t>(n, 1)]) {
    for (int64_t i = 0; i < n; ++i) final_[(size_t)i].store(false, std::memory_order_relaxed);
  }
  void mark_final(int64_t i) { final_[(size_t)i].store(true, std::memory_order_release); }
  bool is_final(int64_t i) const { return final_[(size_t)i].load(std::memory_order_acquire); }
  bool done() const { return next_ >= n_; }
  // the next item if it is below `limit` and final (it counts as handed on), else -1
  int64_t take(int64_t limit) { return next_ < std::min(limit, n_) && is_final(next_) ? next_++ : -1; }
  void wait_next(InflightWindow& window) {
    if (!done()) window.wait_for([&] { return is_final(next_); });
  }

 private:
  const int64_t n_;
  std::unique_ptr<std::atomic<bool>[]> final_;
  int64_t next_ = 0;
};

// The first error of the pipeline's threads: its code and the pipeline's own text for it (text == nullptr: the call that
// failed has left its own).  Read by the calling thread after the joins.
class FirstError {
 public:
  void set(int code, const char* text) {
    std::lock_guard<std::mutex> lk(mu_);
    if (code_.load() != 0) return;
    if (text) { text_ = text; has_text_ = true; }
    code_.store(code);
  }
  int code() const { return code_.load(); }
  const char* text() const { return has_text_ ? text_.c_str() : nullptr; }  // after the joins

 private:
  std::mutex mu_;
  std::atomic<int> code_{0};
  std::string text_;
  bool has_text_ = false;
};

// Owns the three thread groups over their three hand-offs and ends them in the one order that works:
//  * the device threads are joined BEFORE the streamer's list is closed: until then the device may hand items back to it;
//  * the workers' list is closed by the streamer when it has passed on its last chunk, or by close_feed() when there is no
//    streamer -- which is why an item may only go to the device or the streamer when one was started;
//  * the destructor does both steps, so every thread is joined on every path out of the scope.  Declare it after
//    everything the threads use.
template <class Task, class Item>
class StageThreads {
 public:
  StageThreads(Handoff<Task>& work, Handoff<Item>& to_stream, Handoff<Item>& to_device) : work_(work), to_stream_(to_stream), to_device_(to_device) {}
  StageThreads(const StageThreads&) = delete;
  StageThreads& operator=(const StageThreads&) = delete;
  ~StageThreads() { close_feed(); join(); }
  template <class Entry>
  void start_workers(int n, Entry entry) { for (int t = 0; t < n; ++t) workers_.emplace_back(entry); }
  template <class Entry>
  void start_device(int n, Entry entry) { for (int t = 0; t < n; ++t) device_.emplace_back(entry, t); }
  template <class Entry>
  void start_streamer(Entry entry) {
    streamer_ = std::thread([this, entry] { entry(); work_.close(); });
    has_streamer_ = true;
  }
  // the feeder has routed its last item: nothing more for the device, then nothing more for the streamer
  void close_feed() {
    to_device_.close();
    for (auto& t : device_) if (t.joinable()) t.join();
    to_stream_.close();
    if (!has_streamer_) work_.close();
  }
  void join() {
    if (streamer_.joinable()) streamer_.join();
    for (auto& t : workers_) if (t.joinable()) t.join();
  }
  bool all_joined() const {
    for (auto& t : workers_) if (t.joinable()) return false;
    for (auto& t : device_) if (t.joinable()) return false;
    return !streamer_.joinable();
  }

 private:
  Handoff<Task>& work_;
  Handoff<Item>& to_stream_;
  Handoff<Item>& to_device_;
  std::vector<std::thread> workers_, device_;
  std::thread streamer_;
  bool has_streamer_ = false;
};

}  // namespace skch
