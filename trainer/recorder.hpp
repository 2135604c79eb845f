// Episode files from the library's episode recorders (aleppo_rec_open / aleppo_rec_count / aleppo_rec_read /
// aleppo_rec_clear): what the reference's EpisodeRecorder / EpisodeObservationRecorder around environment 0 write
// (src/ai/rollout.cc:149-158), without ffmpeg.  Per episode two files in the video directory:
//   <name>.y4m  uncompressed YUV4MPEG2, "YUV4MPEG2 W<w> H<h> F<f>:1 Ip A1:1 Cmono\n", then per frame "FRAME\n" + w*h bytes:
//               84x84 content at 15 frames/s (one frame per agent step = four emulator frames at 60 Hz), raw pairs as
//               160x210 at 30 frames/s (both frames of each pair in order, each byte through the gray LUT)
//   <name>.tsv  one line per step: ordinal action reward value start terminated truncated game_over lives logit_0 ..
//               logit_{A-1}, tab-separated, floats as %.9g
// A file is opened at a row with start = 1 and closed after a row with terminated or truncated; it is written as
// <name>.part and renamed on close.  Rows before the first start row, and an episode with a gap in its ordinals (steps the
// log dropped or the host drove), are skipped.  n counts the source's episodes from 1, skipped ones included; only episodes
// 1, N + 1, 2 N + 1, ... (record_interval: N) are written, and only their content rows are read from the device - every
// step's 32-byte record is.
#pragma once
#include "../include/aleppo.h"
#include <cstdio>
#include <filesystem>
#include <stdexcept>
#include <string>
#include <vector>

// weak like the other optional entry points (train.cc): a library without them refuses the keys at start-up
#pragma weak aleppo_rec_open
#pragma weak aleppo_rec_count
#pragma weak aleppo_rec_read
#pragma weak aleppo_rec_clear

class EpisodeWriter {
public:
  // prefix: "episode_" or "eval_<step>_episode_"; field: ALEPPO_REC_F_FRAMES or ALEPPO_REC_F_OBSERVATIONS; raw: the field's
  // rows are raw pairs; continue_numbering: n starts after the highest <prefix><n> already in dir (a resumed run)
  EpisodeWriter(std::string dir, std::string prefix, int source, int field, bool raw, size_t actions, size_t interval,
                const uint8_t *lut256, bool continue_numbering)
      : dir_(std::move(dir)), prefix_(std::move(prefix)), source_(source), field_(field), raw_(raw), A_(actions),
        interval_(interval ? interval : 1) {
    for (int i = 0; i < 256; ++i)
      lut_[i] = lut256 ? lut256[i] : (uint8_t)i;
    std::filesystem::create_directories(dir_);
    if (continue_numbering)
      for (const auto &e : std::filesystem::directory_iterator(dir_)) {
        const std::string f = e.path().filename().string();
        if (f.compare(0, prefix_.size(), prefix_) == 0 && f.size() > prefix_.size() && isdigit((unsigned char)f[prefix_.size()]))
          n_ = std::max(n_, (size_t)std::strtoull(f.c_str() + prefix_.size(), nullptr, 10));
      }
  }
  EpisodeWriter(const EpisodeWriter &) = delete;
  EpisodeWriter &operator=(const EpisodeWriter &) = delete;
  ~EpisodeWriter() { close_files(false, false); } // (an unfinished episode stays a .part)

  // read the log's step records, write the selected episodes' rows, clear the log.  check: the caller's error handler
  template <class Check> void drain(aleppo_ctx *ctx, Check &&check) {
    aleppo_rec_counts n{};
    check(ctx, aleppo_rec_count(ctx, source_, &n));
    if (n.dropped && in_episode_)
      broken();
    std::vector<aleppo_rec_step> st((size_t)n.rows);
    if (n.rows)
      check(ctx, aleppo_rec_read(ctx, source_, ALEPPO_REC_F_STEPS, 0, n.rows, st.data(), st.size() * sizeof(aleppo_rec_step)));
    const size_t row_bytes = (size_t)(field_ == ALEPPO_REC_F_FRAMES ? n.frame_bytes : n.observation_bytes);
    size_t r = 0;
    while (r < st.size()) {
      if (st[r].start) { // a new episode (an open one without its end: it was not recorded whole)
        if (in_episode_)
          broken();
        begin();
      } else if (!in_episode_) { // in front of the first start row
        ++r;
        continue;
      } else if (st[r].ordinal != last_ordinal_ + 1) {
        broken();
      }
      size_t e = r; // the episode's rows in this drain: [r, e]
      bool ended = false;
      for (;;) {
        if (st[e].terminated || st[e].truncated) {
          ended = true;
          break;
        }
        if (e + 1 >= st.size() || st[e + 1].start || st[e + 1].ordinal != st[e].ordinal + 1)
          break;
        ++e;
      }
      last_ordinal_ = st[e].ordinal;
      if (y4m_) {
        const size_t rows = e - r + 1;
        content_.resize(rows * row_bytes);
        logits_.resize(rows * A_);
        check(ctx, aleppo_rec_read(ctx, source_, field_, r, rows, content_.data(), content_.size()));
        check(ctx, aleppo_rec_read(ctx, source_, ALEPPO_REC_F_LOGITS, r, rows, logits_.data(), logits_.size() * sizeof(float)));
        for (size_t k = 0; k < rows; ++k)
          write_row(st[r + k], content_.data() + k * row_bytes, logits_.data() + k * A_);
      }
      if (ended) {
        close_files(true, false);
        in_episode_ = false;
      }
      r = e + 1;
    }
    check(ctx, aleppo_rec_clear(ctx, source_));
  }
  // the unfinished episode at the end of an evaluation: its .part files are removed
  void discard() {
    close_files(false, true);
    in_episode_ = false;
  }
  size_t episodes() const { return n_; }

private:
  void begin() {
    in_episode_ = true;
    ++n_;
    if ((n_ - 1) % interval_)
      return;
    base_ = dir_ + "/" + prefix_ + std::to_string(n_);
    y4m_ = std::fopen((base_ + ".y4m.part").c_str(), "wb");
    tsv_ = std::fopen((base_ + ".tsv.part").c_str(), "w");
    if (!y4m_ || !tsv_)
      throw std::runtime_error("cannot write episode files under " + dir_);
    if (raw_)
      std::fprintf(y4m_, "YUV4MPEG2 W160 H210 F30:1 Ip A1:1 Cmono\n");
    else
      std::fprintf(y4m_, "YUV4MPEG2 W84 H84 F15:1 Ip A1:1 Cmono\n");
  }
  void broken() { close_files(false, true); } // (the episode stays counted; the rest of its rows are skipped)
  void write_row(const aleppo_rec_step &s, const uint8_t *px, const float *logits) {
    if (raw_) {
      uint8_t frame[210 * 160];
      for (int k = 0; k < 2; ++k) {
        for (size_t i = 0; i < sizeof frame; ++i)
          frame[i] = lut_[px[k * sizeof frame + i]];
        std::fwrite("FRAME\n", 1, 6, y4m_);
        std::fwrite(frame, 1, sizeof frame, y4m_);
      }
    } else {
      std::fwrite("FRAME\n", 1, 6, y4m_);
      std::fwrite(px, 1, 84 * 84, y4m_);
    }
    std::fprintf(tsv_, "%llu\t%d\t%.9g\t%.9g\t%d\t%d\t%d\t%d\t%d", (unsigned long long)s.ordinal, (int)s.action, (double)s.reward,
                 (double)s.value, (int)s.start, (int)s.terminated, (int)s.truncated, (int)s.game_over, (int)s.lives);
    for (size_t a = 0; a < A_; ++a)
      std::fprintf(tsv_, "\t%.9g", (double)logits[a]);
    std::fputc('\n', tsv_);
  }
  void close_files(bool finished, bool remove) {
    if (!y4m_ && !tsv_)
      return;
    if (y4m_)
      std::fclose(y4m_);
    if (tsv_)
      std::fclose(tsv_);
    y4m_ = tsv_ = nullptr;
    std::error_code ec;
    for (const char *ext : {".y4m", ".tsv"}) {
      if (finished)
        std::filesystem::rename(base_ + ext + ".part", base_ + ext, ec);
      else if (remove)
        std::filesystem::remove(base_ + ext + ".part", ec);
    }
  }

  const std::string dir_, prefix_;
  const int source_, field_;
  const bool raw_;
  const size_t A_, interval_;
  uint8_t lut_[256];
  size_t n_ = 0;
  bool in_episode_ = false;
  uint64_t last_ordinal_ = 0;
  std::string base_;
  std::FILE *y4m_ = nullptr, *tsv_ = nullptr;
  std::vector<uint8_t> content_;
  std::vector<float> logits_;
};
