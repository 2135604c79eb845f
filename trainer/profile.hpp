// [profile] argument: host spans + roctx ranges
#pragma once
#include "../include/aleppo.h"
#include <chrono>
#include <dlfcn.h>
#include <fstream>
#include <string>
#include <vector>

class Profile {
public:
  explicit Profile(const std::string &path) : path_(path), t0_(std::chrono::steady_clock::now()) {
    if (path_.empty())
      return;
    if (void *h = dlopen("libroctx64.so", RTLD_NOW | RTLD_GLOBAL)) { // optional: markers for rocprofv3 --marker-trace
      push_ = reinterpret_cast<int (*)(const char *)>(dlsym(h, "roctxRangePushA"));
      pop_ = reinterpret_cast<int (*)()>(dlsym(h, "roctxRangePop"));
    }
  }
  bool on() const { return !path_.empty(); }
  struct Span {
    Profile *p;
    const char *name;
    double t0;
    Span(Profile *p_, const char *n) : p(p_), name(n), t0(0) {
      if (!p->on())
        return;
      t0 = p->now_us();
      if (p->push_)
        p->push_(name);
    }
    ~Span() {
      if (!p->on())
        return;
      if (p->pop_)
        p->pop_();
      p->events_.push_back({name, t0, p->now_us() - t0});
    }
  };
  void device_summary(aleppo_ctx *ctx) { // per-kernel-class device time (HIP events on the kernels' streams)
    static const char *names[ALEPPO_K_COUNT] = {"ingest", "gae", "head", "adam", "conv1_fwd", "conv2_fwd", "conv3_fwd",
                                                "fc_fwd", "fc_dgrad", "fc_wgrad", "conv3_dgrad", "conv3_wgrad",
                                                "conv2_dgrad", "conv2_wgrad", "conv1_wgrad", "reduce", "infer_head",
                                                "act_fused", "conv_fwd", "conv_bwd", "rec_capture", "act_stats",
                                                "recycle", "sal_blur", "sal_perturb", "sal_score", "ema"};
    for (int k = 0; k < ALEPPO_K_COUNT; ++k) {
      double ms = 0;
      int64_t n = 0;
      if (aleppo_profile_read(ctx, k, &ms, &n) == ALEPPO_OK && n > 0)
        device_.push_back({names[k], ms, n});
    }
  }
  void save() {
    if (!on())
      return;
    std::ofstream f(path_);
    f << "{\"traceEvents\": [\n";
    bool first = true;
    for (auto &e : events_) {
      f << (first ? "" : ",\n") << "{\"name\": \"" << e.name << "\", \"ph\": \"X\", \"pid\": 1, \"tid\": 1, \"ts\": "
        << e.ts << ", \"dur\": " << e.dur << "}";
      first = false;
    }
    f << "\n],\n\"device_kernel_classes\": [\n";
    first = true;
    for (auto &d : device_) {
      f << (first ? "" : ",\n") << "{\"kernel_class\": \"" << d.name << "\", \"avg_ms\": " << d.ms
        << ", \"launches\": " << d.n << "}";
      first = false;
    }
    f << "\n]}\n";
  }

private:
  friend struct Span;
  double now_us() const { return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0_).count(); }
  struct Ev {
    const char *name;
    double ts, dur;
  };
  struct Dev {
    const char *name;
    double ms;
    int64_t n;
  };
  std::string path_;
  std::chrono::steady_clock::time_point t0_;
  int (*push_)(const char *) = nullptr;
  int (*pop_)() = nullptr;
  std::vector<Ev> events_;
  std::vector<Dev> device_;
};
