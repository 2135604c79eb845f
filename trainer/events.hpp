// TensorBoard event file (TFRecord + protobuf by hand)
#pragma once
#include <algorithm>
#include <chrono>
#include <cstdint>
#include <fstream>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

static uint32_t crc32c(const uint8_t *p, size_t n) {
  static uint32_t table[256];
  static bool init = false;
  if (!init) {
    for (uint32_t i = 0; i < 256; ++i) {
      uint32_t c = i;
      for (int k = 0; k < 8; ++k)
        c = (c & 1) ? (c >> 1) ^ 0x82F63B78u : c >> 1;
      table[i] = c;
    }
    init = true;
  }
  uint32_t c = 0xFFFFFFFFu;
  for (size_t i = 0; i < n; ++i)
    c = table[(c ^ p[i]) & 255] ^ (c >> 8);
  return c ^ 0xFFFFFFFFu;
}
static uint32_t masked_crc(const uint8_t *p, size_t n) {
  const uint32_t c = crc32c(p, n);
  return ((c >> 15) | (c << 17)) + 0xa282ead8u;
}
struct Pb { // minimal protobuf encoder
  std::string b;
  void varint(uint64_t v) {
    while (v >= 128) {
      b.push_back((char)(v | 128));
      v >>= 7;
    }
    b.push_back((char)v);
  }
  void key(int field, int wire) { varint(((uint64_t)field << 3) | wire); }
  void f64(int field, double v) {
    key(field, 1);
    b.append(reinterpret_cast<const char *>(&v), 8);
  }
  void f32(int field, float v) {
    key(field, 5);
    b.append(reinterpret_cast<const char *>(&v), 4);
  }
  void i64(int field, int64_t v) {
    key(field, 0);
    varint((uint64_t)v);
  }
  void bytes(int field, const std::string &s) {
    key(field, 2);
    varint(s.size());
    b += s;
  }
  void packed_f64(int field, const std::vector<double> &v) {
    key(field, 2);
    varint(v.size() * 8);
    b.append(reinterpret_cast<const char *>(v.data()), v.size() * 8);
  }
};
class EventWriter {
public:
  explicit EventWriter(const std::string &path) : f_(path, std::ios::binary) {
    if (!f_)
      throw std::runtime_error("cannot open event file: " + path);
    Pb e;
    e.f64(1, now());
    e.bytes(3, "brain.Event:2"); // file_version
    record(e.b);
  }
  void add_scalar(const std::string &tag, int64_t step, float value) {
    Pb v;
    v.bytes(1, tag);
    v.f32(2, value);
    summary_event(v, &step);
  }
  void add_histogram(const std::string &tag, int64_t step, const std::vector<float> &x) {
    if (x.empty())
      return;
    double mn = x[0], mx = x[0], sum = 0, sq = 0;
    for (float v : x) {
      mn = std::min<double>(mn, v);
      mx = std::max<double>(mx, v);
      sum += v;
      sq += (double)v * v;
    }
    const int nb = 30;
    std::vector<double> limits(nb), counts(nb, 0.0);
    const double w = (mx - mn) / nb > 0 ? (mx - mn) / nb : 1.0;
    for (int i = 0; i < nb; ++i)
      limits[i] = mn + w * (i + 1);
    for (float v : x)
      counts[std::min(nb - 1, (int)((v - mn) / w))] += 1.0;
    Pb h; // HistogramProto: min=1 max=2 num=3 sum=4 sum_squares=5 bucket_limit=6 bucket=7
    h.f64(1, mn);
    h.f64(2, mx);
    h.f64(3, (double)x.size());
    h.f64(4, sum);
    h.f64(5, sq);
    h.packed_f64(6, limits);
    h.packed_f64(7, counts);
    Pb v;
    v.bytes(1, tag);
    v.bytes(5, h.b); // Summary.Value.histo
    summary_event(v, &step);
  }
  // logger.add_hparams(get_parameters(config), group_name, start_time) (src/bin/train.cc:72-105, :389): the HParams
  // plugin's session-start record.  Summary.Value{tag "_hparams_/session_start_info", metadata.plugin_data{plugin_name
  // "hparams", content = HParamsPluginData{version 0, session_start_info{hparams map<string, google.protobuf.Value>,
  // group_name, start_time_secs}}}}
  void add_hparams(const std::vector<std::pair<std::string, double>> &numbers,
                   const std::vector<std::pair<std::string, bool>> &flags, const std::string &group, double start_secs) {
    Pb ssi;
    auto entry = [&](const std::string &k, const Pb &val) {
      Pb kv; // map entry: key = 1, value = 2
      kv.bytes(1, k);
      kv.bytes(2, val.b);
      ssi.bytes(1, kv.b);
    };
    for (auto &n : numbers) {
      Pb v;
      v.f64(2, n.second); // google.protobuf.Value.number_value
      entry(n.first, v);
    }
    for (auto &b : flags) {
      Pb v;
      v.i64(4, b.second ? 1 : 0); // google.protobuf.Value.bool_value
      entry(b.first, v);
    }
    ssi.bytes(4, group);
    ssi.f64(5, start_secs);
    Pb plugin; // HParamsPluginData: version = 1, session_start_info = 3
    plugin.i64(1, 0);
    plugin.bytes(3, ssi.b);
    Pb pd; // SummaryMetadata.PluginData: plugin_name = 1, content = 2
    pd.bytes(1, "hparams");
    pd.bytes(2, plugin.b);
    Pb md; // SummaryMetadata: plugin_data = 1
    md.bytes(1, pd.b);
    Pb v; // Summary.Value: tag = 1, metadata = 9
    v.bytes(1, "_hparams_/session_start_info");
    v.bytes(9, md.b);
    summary_event(v, nullptr);
  }
  void flush() { f_.flush(); }

private:
  static double now() { return std::chrono::duration<double>(std::chrono::system_clock::now().time_since_epoch()).count(); }
  void summary_event(const Pb &value, const int64_t *step) { // Event{wall_time, [step,] summary{value}}
    Pb s;
    s.bytes(1, value.b);
    Pb e;
    e.f64(1, now());
    if (step)
      e.i64(2, *step);
    e.bytes(5, s.b);
    record(e.b);
  }
  void record(const std::string &data) {
    const uint64_t len = data.size();
    const uint32_t c1 = masked_crc(reinterpret_cast<const uint8_t *>(&len), 8);
    const uint32_t c2 = masked_crc(reinterpret_cast<const uint8_t *>(data.data()), data.size());
    f_.write(reinterpret_cast<const char *>(&len), 8);
    f_.write(reinterpret_cast<const char *>(&c1), 4);
    f_.write(data.data(), (std::streamsize)data.size());
    f_.write(reinterpret_cast<const char *>(&c2), 4);
  }
  std::ofstream f_;
};
