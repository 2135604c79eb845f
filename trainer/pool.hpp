// Worker pool (std::thread + index queue, rollout.cc:280-297)
#pragma once
#include <condition_variable>
#include <functional>
#include <mutex>
#include <thread>
#include <vector>

class WorkerPool {
public:
  explicit WorkerPool(size_t n) {
    for (size_t i = 0; i < n; ++i)
      threads_.emplace_back([this] { loop(); });
  }
  ~WorkerPool() {
    {
      std::lock_guard<std::mutex> l(m_);
      stop_ = true;
    }
    cv_.notify_all();
    for (auto &t : threads_)
      t.join();
  }
  // push indices 0..count-1, the workers call fn on each; wait until all are done (step_all)
  void run_all(size_t count, const std::function<void(size_t)> &fn) {
    {
      std::lock_guard<std::mutex> l(m_);
      fn_ = &fn;
      next_ = 0;
      end_ = count;
      done_ = 0;
    }
    cv_.notify_all();
    std::unique_lock<std::mutex> l(m_);
    done_cv_.wait(l, [&] { return done_ == end_; });
  }

private:
  void loop() {
    for (;;) {
      size_t i;
      const std::function<void(size_t)> *fn;
      {
        std::unique_lock<std::mutex> l(m_);
        cv_.wait(l, [&] { return stop_ || next_ < end_; });
        if (stop_)
          return;
        i = next_++;
        fn = fn_;
      }
      (*fn)(i);
      {
        std::lock_guard<std::mutex> l(m_);
        if (++done_ == end_)
          done_cv_.notify_all();
      }
    }
  }
  const std::function<void(size_t)> *fn_ = nullptr; // the job of the run_all in progress
  std::vector<std::thread> threads_;
  std::mutex m_;
  std::condition_variable cv_, done_cv_;
  size_t next_ = 0, end_ = 0, done_ = 0;
  bool stop_ = false;
};
