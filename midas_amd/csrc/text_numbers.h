// float() / int() of a text field as the readers of this library take them (genes_merge_io.cpp, sites_io.cpp): ASCII
// whitespace trimmed, plain decimals and the nan / inf / infinity spellings.  parse_f64_py / parse_i64_py also take the
// digit separators Python allows ('1_000': an underscore between two digits).
#pragma once
#include <charconv>
#include <cstdint>
#include <cstdlib>
#include <string>
#include <string_view>

namespace midas {

inline bool py_space(char c) { return c == ' ' || (c >= '\t' && c <= '\r') || (c >= 0x1c && c <= 0x1f); }

inline std::string_view trim(std::string_view v) {
  size_t a = 0, b = v.size();
  while (a < b && py_space(v[a])) ++a;
  while (b > a && py_space(v[b - 1])) --b;
  return v.substr(a, b - a);
}

// float(field): true and *out, or false for a spelling this build does not take
inline bool parse_f64(std::string_view v, double* out) {
  v = trim(v);
  if (v.empty()) return false;
  size_t i = 0;
  if (v[0] == '+' || v[0] == '-') i = 1;
  if (i >= v.size() || v[i] == '+' || v[i] == '-') return false;
  for (char c : v)
    if (c == '(' || c == '_') return false;       // nan(...) / digit separators
  const std::string_view body = v.substr(i);
  double x = 0.0;
  const auto r = std::from_chars(body.data(), body.data() + body.size(), x, std::chars_format::general);
  if (r.ptr != body.data() + body.size()) return false;
  if (r.ec == std::errc::result_out_of_range) {    // overflow -> inf, underflow -> 0 (Python's float())
    const std::string z(body);
    x = strtod(z.c_str(), nullptr);
  } else if (r.ec != std::errc()) {
    return false;
  }
  *out = v[0] == '-' ? -x : x;
  return true;
}

inline bool parse_i64(std::string_view v, int64_t* out) {
  v = trim(v);
  size_t i = 0;
  if (!v.empty() && (v[0] == '+' || v[0] == '-')) i = 1;
  if (i >= v.size()) return false;
  for (size_t k = i; k < v.size(); ++k)
    if (v[k] < '0' || v[k] > '9') return false;
  uint64_t u = 0;
  const auto r = std::from_chars(v.data() + i, v.data() + v.size(), u);
  if (r.ec != std::errc() || r.ptr != v.data() + v.size()) return false;
  if (v[0] == '-') {
    if (u > (uint64_t)1 << 63) return false;
    *out = (int64_t)(0 - u);
  } else {
    if (u > (uint64_t)INT64_MAX) return false;
    *out = (int64_t)u;
  }
  return true;
}

// v without its underscores when every one of them stands between two digits; false otherwise
inline bool strip_digit_separators(std::string_view v, std::string* out) {
  out->clear();
  for (size_t k = 0; k < v.size(); ++k) {
    if (v[k] != '_') { out->push_back(v[k]); continue; }
    const bool l = k > 0 && v[k - 1] >= '0' && v[k - 1] <= '9', r = k + 1 < v.size() && v[k + 1] >= '0' && v[k + 1] <= '9';
    if (!l || !r) return false;
  }
  return true;
}

inline bool parse_f64_py(std::string_view v, double* out) {
  if (v.find('_') == std::string_view::npos) return parse_f64(v, out);
  std::string z;
  return strip_digit_separators(trim(v), &z) && parse_f64(z, out);
}

inline bool parse_i64_py(std::string_view v, int64_t* out) {
  if (v.find('_') == std::string_view::npos) return parse_i64(v, out);
  std::string z;
  return strip_digit_separators(trim(v), &z) && parse_i64(z, out);
}

}  // namespace midas
