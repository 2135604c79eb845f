// Checkpoint file (INTEGRATION.md has the framing; visit_checkpoint below IS the description of what the sections hold)
#pragma once
#include "../include/aleppo.h"
#include "emulator.hpp"
#include <cstdint>
#include <cstring>
#include <filesystem>
#include <fstream>
#include <map>
#include <stdexcept>
#include <string>
#include <type_traits>
#include <vector>

// little-endian: magic, version, the shape header, sections of (u32 id, u64 byte length, bytes), the end mark
constexpr char CKPT_MAGIC[8] = {'A', 'L', 'E', 'P', 'P', 'O', 'C', 'K'};
constexpr char CKPT_END[8] = {'A', 'L', 'E', 'P', 'P', 'O', 'E', 'N'};
constexpr uint32_t CKPT_VERSION = 1;
enum CkptSection : uint32_t { CK_PARAMS = 1, CK_OPTIMIZER = 2, CK_REWARD_SCALE = 3, CK_ROLLOUT = 4, CK_TRAINER = 5, CK_DIGEST = 6,
                              CK_EMA = 7,   // (CK_EMA is optional: written only by runs with ema_decay, ignored by runs without)
                              CK_ANCHOR = 8 }; // (optional like CK_EMA: written only by runs with l2_init_coef > 0, which need it to resume)
static const char *const DIGEST_NAMES[ALEPPO_DIGEST_COUNT] = {"params", "optimizer", "rollout", "reward_scale"};
struct CkptShape {
  uint32_t E, T, A, H, precision, world, rank, reserved;
  uint64_t param_count;
};
struct Checkpoint {
  CkptShape shape{};
  std::map<uint32_t, std::string> sections;
};
template <class T> static void put(std::string &out, const T &v) { out.append(reinterpret_cast<const char *>(&v), sizeof(T)); }
// the bytes of the optional section CK_EMA: the averaged parameters (aleppo_ema_export, reference order), then u64 updates.
// It is outside visit_checkpoint: the format version stays 1 and the files of runs without ema_decay stay byte-identical.
static std::string ema_section(const std::vector<float> &avg, uint64_t updates) {
  std::string s(reinterpret_cast<const char *>(avg.data()), avg.size() * sizeof(float));
  put(s, updates);
  return s;
}
// the bytes of the optional section CK_ANCHOR: the anchor of l2_init_coef (aleppo_anchor_export, reference order).  Outside
// visit_checkpoint like CK_EMA: the files of runs without the key stay byte-identical.
static std::string anchor_section(const std::vector<float> &anchor) {
  return std::string(reinterpret_cast<const char *>(anchor.data()), anchor.size() * sizeof(float));
}
// What the library exports and imports (the learner's sections and the digest) ...
struct DeviceState {
  std::vector<float> params, exp_avg, exp_avg_sq;
  int64_t adam_step = 0;
  std::vector<double> reward_scale; // 3 statistics, then the environments' running returns
  uint64_t rollout_words[ALEPPO_ROLLOUT_STATE_WORDS] = {};
  std::vector<uint8_t> observations;
  uint64_t digest[ALEPPO_DIGEST_COUNT] = {};
  DeviceState(size_t n, size_t E) : params(n), exp_avg(n), exp_avg_sq(n), reward_scale(3 + E), observations(E * 4 * 84 * 84) {}
};
// ... and the trainer's own bookkeeping between two rollouts (src/ai/rollout.cc:204-267), down to every emulator's fields
struct TrainerState {
  uint64_t next_rollout = 0, total_steps = 0, episodes = 0;
  uint64_t schedule_position = 0; // the rollout index the annealed values are functions of: always next_rollout
  float kl_beta = 0.0f;
  EnvSet set; // the training environments and their episode-start flags
  std::vector<uint8_t> term, trunc, game_over;
  std::vector<float> rewards, ep_ret, game_ret;
  std::vector<uint64_t> ep_len, game_len;
  explicit TrainerState(size_t E)
      : set(E), term(E, 0), trunc(E, 0), game_over(E, 0), rewards(E, 0.f), ep_ret(E, 0.f), game_ret(E, 0.f), ep_len(E, 0),
        game_len(E, 0) {}
};
// Format version 1, field by field: the writer, the reader and the expected section sizes are all this one function.
// v.section(id, fields...) is a section made of the fields' bytes in order: a scalar's or an array's own bytes, a vector's
// elements without a length (the shape header fixes every length).
template <class V> static void visit_checkpoint(V &v, DeviceState &d, TrainerState &t) {
  v.section(CK_PARAMS, d.params);
  v.section(CK_OPTIMIZER, d.exp_avg, d.exp_avg_sq, d.adam_step);
  v.section(CK_REWARD_SCALE, d.reward_scale);
  v.section(CK_ROLLOUT, d.rollout_words, d.observations);
  v.section(CK_TRAINER, t.next_rollout, t.total_steps, t.episodes, t.schedule_position, t.kl_beta, t.set.start, t.term,
            t.trunc, t.game_over, t.rewards, t.ep_ret, t.game_ret, t.ep_len, t.game_len);
  for (SyntheticAtari &e : t.set.envs)
    e.visit(v);
  v.section(CK_DIGEST, d.digest);
}
template <class Self> struct CkptVisitor { // fields in terms of Self::begin(section id) and Self::raw(pointer, bytes)
  template <class... T> void section(uint32_t id, T &...x) {
    static_cast<Self *>(this)->begin(id);
    (*this)(x...);
  }
  template <class... T> void operator()(T &...x) { (field(x), ...); }
  template <class T> void field(T &x) {
    static_assert(std::is_trivially_copyable<T>::value, "a field is its own bytes");
    static_cast<Self *>(this)->raw(&x, sizeof(T));
  }
  template <class T> void field(std::vector<T> &x) { static_cast<Self *>(this)->raw(x.data(), x.size() * sizeof(T)); }
};
struct CkptWriter : CkptVisitor<CkptWriter> {
  std::map<uint32_t, std::string> &sections;
  std::string *out = nullptr;
  explicit CkptWriter(std::map<uint32_t, std::string> &s) : sections(s) {}
  void begin(uint32_t id) { out = &sections[id]; }
  void raw(const void *p, size_t n) { out->append(static_cast<const char *>(p), n); }
};
struct CkptReader : CkptVisitor<CkptReader> { // (of sections whose sizes check_checkpoint_shape has checked)
  const std::map<uint32_t, std::string> &sections;
  const char *in = nullptr;
  explicit CkptReader(const std::map<uint32_t, std::string> &s) : sections(s) {}
  void begin(uint32_t id) { in = sections.at(id).data(); }
  void raw(void *p, size_t n) {
    std::memcpy(p, in, n);
    in += n;
  }
};
static void write_checkpoint_file(const std::string &path, const Checkpoint &ck) {
  std::string out(CKPT_MAGIC, 8);
  put(out, CKPT_VERSION);
  put(out, ck.shape);
  for (const auto &sec : ck.sections) {
    put(out, sec.first);
    put(out, (uint64_t)sec.second.size());
    out += sec.second;
  }
  out.append(CKPT_END, 8);
  const std::string tmp = path + ".tmp";
  {
    std::ofstream f(tmp, std::ios::binary | std::ios::trunc);
    f.write(out.data(), (std::streamsize)out.size());
    f.flush();
    if (!f)
      throw std::runtime_error("cannot write checkpoint " + tmp);
  }
  std::filesystem::rename(tmp, path); // atomic: a reader sees a whole checkpoint under the final name, or the old one
}
// reads and checks the framing: every failure names the file and what is wrong with it
static Checkpoint read_checkpoint_file(const std::string &path) {
  std::ifstream f(path, std::ios::binary);
  if (!f)
    throw std::runtime_error("resume: cannot open checkpoint " + path);
  const std::string in((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
  size_t pos = 0;
  auto need = [&](size_t n) {
    if (in.size() - pos < n)
      throw std::runtime_error("resume: checkpoint " + path + " is truncated");
  };
  auto get = [&](void *dst, size_t n) {
    need(n);
    std::memcpy(dst, in.data() + pos, n);
    pos += n;
  };
  char magic[8];
  get(magic, 8);
  if (std::memcmp(magic, CKPT_MAGIC, 8) != 0)
    throw std::runtime_error("resume: " + path + " is not a checkpoint (wrong magic)");
  uint32_t version = 0;
  get(&version, 4);
  if (version != CKPT_VERSION)
    throw std::runtime_error("resume: checkpoint " + path + " has format version " + std::to_string(version) +
                             ", this build reads version " + std::to_string(CKPT_VERSION));
  Checkpoint ck;
  get(&ck.shape, sizeof(ck.shape));
  for (;;) {
    need(8);
    if (std::memcmp(in.data() + pos, CKPT_END, 8) == 0 && in.size() - pos == 8)
      break;
    uint32_t id = 0;
    uint64_t len = 0;
    get(&id, 4);
    get(&len, 8);
    if (len > in.size() - pos)
      throw std::runtime_error("resume: checkpoint " + path + " is truncated");
    ck.sections[id] = in.substr(pos, (size_t)len);
    pos += (size_t)len;
  }
  for (uint32_t id : {CK_PARAMS, CK_OPTIMIZER, CK_REWARD_SCALE, CK_ROLLOUT, CK_TRAINER, CK_DIGEST})
    if (!ck.sections.count(id))
      throw std::runtime_error("resume: checkpoint " + path + " lacks section " + std::to_string(id));
  return ck;
}
// the shape the file was written for against this run's; the section sizes that follow from it
static void check_checkpoint_shape(const std::string &path, const Checkpoint &ck, const CkptShape &want) {
  const struct {
    const char *name;
    uint64_t file, run;
  } f[] = {{"total_environments / WORLD_SIZE", ck.shape.E, want.E}, {"horizon", ck.shape.T, want.T},
           {"action_size", ck.shape.A, want.A},                     {"hidden_size", ck.shape.H, want.H},
           {"precision", ck.shape.precision, want.precision},       {"WORLD_SIZE", ck.shape.world, want.world},
           {"RANK", ck.shape.rank, want.rank},                      {"parameter count", ck.shape.param_count, want.param_count}};
  for (const auto &x : f)
    if (x.file != x.run)
      throw std::runtime_error("resume: checkpoint " + path + " was written for " + x.name + " = " +
                               std::to_string(x.file) + ", this run has " + std::to_string(x.run));
  // the section sizes that follow: those of a blank state of this run's shape, as the writer itself lays it out
  DeviceState d((size_t)want.param_count, want.E);
  TrainerState t(want.E);
  t.set.envs.assign(want.E, SyntheticAtari(0, 0, 0.f, 0));
  Checkpoint blank;
  CkptWriter out(blank.sections);
  visit_checkpoint(out, d, t);
  for (const auto &sec : blank.sections)
    if (ck.sections.at(sec.first).size() != sec.second.size())
      throw std::runtime_error("resume: checkpoint " + path + " is corrupt (section " + std::to_string(sec.first) +
                               " has " + std::to_string(ck.sections.at(sec.first).size()) + " bytes, expected " +
                               std::to_string(sec.second.size()) + ")");
}
static size_t reference_param_count(size_t H, size_t A) { // libtorch parameters() element count of the network
  return 32 * 256 + 32 + 64 * 512 + 64 + 64 * 576 + 64 + H * 3136 + H + A * H + A + H + 1;
}
