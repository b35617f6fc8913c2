// The host readers under snp_diversity.py / call_consensus.py: one species directory of `merge_midas.py snps`.
//
//   snps_summary.txt  sample_id, mean_coverage, fraction_covered per row; a sample's matrix column is its row index
//                     (fetch_samples, midas/analyze/parse_snps.py:181-194);
//   snps_info.txt     as columns: site_id, ref_allele, major_allele, minor_allele, locus_type, site_type and a gene index
//                     (gene ids numbered in order of first appearance, -1 for an empty id);
//   snps_freq.txt, snps_depth.txt   mapped, NOT parsed: their rows go to the device as bytes (sites_rows.h).  The header
//                     row gives the sample ids; the reference keeps the depth file's (parse_snps.py:55-58).
//
// strain_tracking.py's two output tables are written here too (midas_sites_write_markers / _pairs): integers and strings.
//
// Fields are taken as csv.DictReader(delimiter='\t') takes them from a file opened in text mode: a line ends at '\n'
// ('\r\n' counts as one), an empty line is skipped, a field is the value of the LAST header column of its name, a row with
// fewer fields than the header lacks the later ones (an error here when a needed one is missing).  Quoted fields are not
// interpreted: the merge never writes a quote.
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <charconv>
#include <cstdio>
#include <cstring>
#include <string>
#include <string_view>
#include <unordered_map>
#include <vector>

#include "../../include/midas_snps.h"
#include "text_numbers.h"

namespace {

struct StrCol {        // strings back to back + offsets
  std::vector<char> pool;
  std::vector<int64_t> off{0};
  void push(std::string_view v) {
    pool.insert(pool.end(), v.begin(), v.end());
    off.push_back((int64_t)pool.size());
  }
  std::string_view at(size_t k) const { return std::string_view(pool.data() + off[k], (size_t)(off[k + 1] - off[k])); }
};

// a text file written through a buffer of its own
struct TextOut {
  FILE* f = nullptr;
  std::string buf;
  ~TextOut() { if (f) fclose(f); }
  bool open(const char* path) {
    f = fopen(path, "w");
    buf.reserve(1 << 20);
    return f != nullptr;
  }
  bool flush() {
    const bool ok = buf.empty() || fwrite(buf.data(), 1, buf.size(), f) == buf.size();
    buf.clear();
    return ok;
  }
  void room() { if (buf.size() > (1u << 20) - 4096) bad = !flush() || bad; }
  void put(std::string_view v) { buf.append(v.data(), v.size()); room(); }
  void put(char c) { buf.push_back(c); }
  void put_int(int64_t v) {
    char tmp[24];
    const auto r = std::to_chars(tmp, tmp + sizeof tmp, v);
    buf.append(tmp, (size_t)(r.ptr - tmp));
  }
  bool close() {
    bool ok = flush() && !bad;
    ok = fclose(f) == 0 && ok;
    f = nullptr;
    return ok;
  }
  bool bad = false;
};

struct Mapped {
  const char* base = nullptr;
  size_t size = 0;
  size_t body = 0;       // offset of the first byte after the header line
  ~Mapped() { if (base && size) munmap(const_cast<char*>(base), size); }
  bool open(const char* path) {
    const int fd = ::open(path, O_RDONLY);
    if (fd < 0) return false;
    struct stat st;
    if (fstat(fd, &st) != 0) { ::close(fd); return false; }
    size = (size_t)st.st_size;
    if (size) {
      void* p = mmap(nullptr, size, PROT_READ, MAP_PRIVATE, fd, 0);
      if (p == MAP_FAILED) { ::close(fd); size = 0; return false; }
      base = static_cast<const char*>(p);
    }
    ::close(fd);
    return true;
  }
};

void fail(char* err1024, const std::string& path, long long line, const char* what) {
  if (!err1024) return;
  if (line > 0) snprintf(err1024, 1024, "%s, line %lld: %s", path.c_str(), line, what);
  else snprintf(err1024, 1024, "%s: %s", path.c_str(), what);
}

void split_tabs(std::string_view line, std::vector<std::string_view>* f) {
  f->clear();
  size_t p = 0;
  for (size_t q = 0;; ++q) {
    if (q == line.size() || line[q] == '\t') {
      f->push_back(line.substr(p, q - p));
      if (q == line.size()) break;
      p = q + 1;
    }
  }
}

// the next line of [p, n) without its '\n' / '\r\n'; false at the end
bool next_line(const char* s, size_t n, size_t* p, std::string_view* out) {
  if (*p >= n) return false;
  const char* nl = static_cast<const char*>(memchr(s + *p, '\n', n - *p));
  size_t e = nl ? (size_t)(nl - s) : n;
  const size_t next = nl ? e + 1 : n;
  if (e > *p && s[e - 1] == '\r') --e;
  *out = std::string_view(s + *p, e - *p);
  *p = next;
  return true;
}

int last_column(const std::vector<std::string_view>& header, const char* name) {
  for (int k = (int)header.size() - 1; k >= 0; --k)
    if (header[(size_t)k] == name) return k;
  return -1;
}

}  // namespace

struct midas_sites_tables {
  StrCol sample_ids;
  std::vector<double> mean_coverage, fraction_covered;
  StrCol site_id, ref_allele, major_allele, minor_allele, locus_type, site_type, gene_ids, matrix_ids;
  std::vector<int32_t> gene;
  int64_t freq_columns = 0;
  Mapped freq, depth;
  std::string dir;
  bool have_positions = false;      // midas_sites_tables_positions has read these
  std::vector<int32_t> contig;
  std::vector<int64_t> ref_pos;
  StrCol contig_names;
};

namespace {

int32_t read_summary(const std::string& path, midas_sites_tables* t, char* err) {
  Mapped m;
  if (!m.open(path.c_str())) { fail(err, path, 0, "cannot be read"); return MIDAS_SNPS_ERR_INVALID_ARG; }
  size_t p = 0;
  std::string_view line;
  std::vector<std::string_view> header, f;
  if (!next_line(m.base, m.size, &p, &line)) { fail(err, path, 0, "is empty"); return MIDAS_SNPS_ERR_BAD_LAYOUT; }
  split_tabs(line, &header);
  const int c_id = last_column(header, "sample_id"), c_cov = last_column(header, "mean_coverage"),
            c_fr = last_column(header, "fraction_covered");
  if (c_id < 0 || c_cov < 0 || c_fr < 0) {
    fail(err, path, 1, "the header lacks sample_id, mean_coverage or fraction_covered");
    return MIDAS_SNPS_ERR_BAD_LAYOUT;
  }
  for (long long ln = 2; next_line(m.base, m.size, &p, &line); ++ln) {
    if (line.empty()) continue;
    split_tabs(line, &f);
    double cov = 0, fr = 0;
    if ((int)f.size() <= std::max(c_id, std::max(c_cov, c_fr)) || !midas::parse_f64_py(f[(size_t)c_cov], &cov) ||
        !midas::parse_f64_py(f[(size_t)c_fr], &fr)) {
      fail(err, path, ln, "mean_coverage / fraction_covered is missing or not a number");
      return MIDAS_SNPS_ERR_BAD_LAYOUT;
    }
    t->sample_ids.push(f[(size_t)c_id]);
    t->mean_coverage.push_back(cov);
    t->fraction_covered.push_back(fr);
  }
  return MIDAS_SNPS_OK;
}

int32_t read_info(const std::string& path, midas_sites_tables* t, char* err) {
  Mapped m;
  if (!m.open(path.c_str())) { fail(err, path, 0, "cannot be read"); return MIDAS_SNPS_ERR_INVALID_ARG; }
  size_t p = 0;
  std::string_view line;
  std::vector<std::string_view> header, f;
  if (!next_line(m.base, m.size, &p, &line)) { fail(err, path, 0, "is empty"); return MIDAS_SNPS_ERR_BAD_LAYOUT; }
  split_tabs(line, &header);
  static const char* names[7] = {"site_id", "ref_allele", "major_allele", "minor_allele", "locus_type", "site_type", "gene_id"};
  StrCol* cols[6] = {&t->site_id, &t->ref_allele, &t->major_allele, &t->minor_allele, &t->locus_type, &t->site_type};
  int c[7], need = 0;
  for (int k = 0; k < 7; ++k) {
    c[k] = last_column(header, names[k]);
    if (c[k] < 0) {
      char what[96];
      snprintf(what, sizeof what, "the header lacks the column %s", names[k]);
      fail(err, path, 1, what);
      return MIDAS_SNPS_ERR_BAD_LAYOUT;
    }
    need = std::max(need, c[k] + 1);
  }
  std::unordered_map<std::string, int32_t> index;
  for (long long ln = 2; next_line(m.base, m.size, &p, &line); ++ln) {
    if (line.empty()) continue;
    split_tabs(line, &f);
    if ((int)f.size() < need) { fail(err, path, ln, "the row has fewer fields than the columns in use"); return MIDAS_SNPS_ERR_BAD_LAYOUT; }
    for (int k = 0; k < 6; ++k) cols[k]->push(f[(size_t)c[k]]);
    const std::string_view g = f[(size_t)c[6]];
    int32_t gi = -1;
    if (!g.empty()) {
      const auto it = index.emplace(std::string(g), (int32_t)index.size());
      gi = it.first->second;
      if (it.second) t->gene_ids.push(g);
    }
    t->gene.push_back(gi);
  }
  return MIDAS_SNPS_OK;
}

// ref_id -> contig index in order of first appearance, ref_pos -> int(): the rows read_info keeps (it skips empty lines)
int32_t read_positions(const std::string& path, midas_sites_tables* t, char* err) {
  Mapped m;
  if (!m.open(path.c_str())) { fail(err, path, 0, "cannot be read"); return MIDAS_SNPS_ERR_INVALID_ARG; }
  size_t p = 0;
  std::string_view line;
  std::vector<std::string_view> header, f;
  if (!next_line(m.base, m.size, &p, &line)) { fail(err, path, 0, "is empty"); return MIDAS_SNPS_ERR_BAD_LAYOUT; }
  split_tabs(line, &header);
  const int c_id = last_column(header, "ref_id"), c_pos = last_column(header, "ref_pos");
  if (c_id < 0 || c_pos < 0) {
    fail(err, path, 1, c_id < 0 ? "the header lacks the column ref_id" : "the header lacks the column ref_pos");
    return MIDAS_SNPS_ERR_BAD_LAYOUT;
  }
  std::vector<int32_t> contig;
  std::vector<int64_t> ref_pos;
  StrCol names;
  std::unordered_map<std::string, int32_t> index;
  for (long long ln = 2; next_line(m.base, m.size, &p, &line); ++ln) {
    if (line.empty()) continue;
    split_tabs(line, &f);
    if ((int)f.size() <= std::max(c_id, c_pos)) { fail(err, path, ln, "the row lacks ref_id or ref_pos"); return MIDAS_SNPS_ERR_BAD_LAYOUT; }
    int64_t pos = 0;
    if (!midas::parse_i64_py(f[(size_t)c_pos], &pos)) { fail(err, path, ln, "ref_pos is not an integer"); return MIDAS_SNPS_ERR_BAD_LAYOUT; }
    const std::string_view id = f[(size_t)c_id];
    const auto it = index.emplace(std::string(id), (int32_t)index.size());
    if (it.second) names.push(id);
    contig.push_back(it.first->second);
    ref_pos.push_back(pos);
  }
  t->contig.swap(contig);
  t->ref_pos.swap(ref_pos);
  t->contig_names = std::move(names);
  t->have_positions = true;
  return MIDAS_SNPS_OK;
}

int32_t map_matrix(const std::string& path, Mapped* m, std::vector<std::string_view>* header, char* err) {
  if (!m->open(path.c_str())) { fail(err, path, 0, "cannot be read"); return MIDAS_SNPS_ERR_INVALID_ARG; }
  size_t p = 0;
  std::string_view line;
  if (!next_line(m->base, m->size, &p, &line)) { fail(err, path, 0, "is empty"); return MIDAS_SNPS_ERR_BAD_LAYOUT; }
  split_tabs(line, header);
  m->body = p;
  return MIDAS_SNPS_OK;
}

}  // namespace

extern "C" {

int32_t midas_sites_tables_open(const char* dir, midas_sites_tables** out, char* err1024) {
  if (!dir || !out) return MIDAS_SNPS_ERR_INVALID_ARG;
  *out = nullptr;
  if (err1024) err1024[0] = 0;
  midas_sites_tables* t = new midas_sites_tables();
  const std::string d(dir);
  std::vector<std::string_view> hf, hd;
  int32_t st = read_summary(d + "/snps_summary.txt", t, err1024);
  if (st == MIDAS_SNPS_OK) st = read_info(d + "/snps_info.txt", t, err1024);
  if (st == MIDAS_SNPS_OK) st = map_matrix(d + "/snps_freq.txt", &t->freq, &hf, err1024);
  if (st == MIDAS_SNPS_OK) st = map_matrix(d + "/snps_depth.txt", &t->depth, &hd, err1024);
  if (st != MIDAS_SNPS_OK) { delete t; return st; }
  t->dir = d;
  t->freq_columns = (int64_t)hf.size() - 1;
  for (size_t k = 1; k < hd.size(); ++k) t->matrix_ids.push(hd[k]);
  *out = t;
  return MIDAS_SNPS_OK;
}

int32_t midas_sites_tables_counts(const midas_sites_tables* t, int64_t* out8) {
  if (!t || !out8) return MIDAS_SNPS_ERR_INVALID_ARG;
  out8[0] = (int64_t)t->mean_coverage.size();
  out8[1] = (int64_t)t->gene.size();
  out8[2] = (int64_t)t->gene_ids.off.size() - 1;
  out8[3] = (int64_t)t->matrix_ids.off.size() - 1;
  out8[4] = (int64_t)(t->freq.size - t->freq.body);
  out8[5] = (int64_t)(t->depth.size - t->depth.body);
  out8[6] = t->freq_columns;
  out8[7] = 0;
  return MIDAS_SNPS_OK;
}

int32_t midas_sites_tables_columns(const midas_sites_tables* t, const void** out25, int64_t* sizes10) {
  if (!t || !out25 || !sizes10) return MIDAS_SNPS_ERR_INVALID_ARG;
  const StrCol* s[10] = {&t->sample_ids, &t->site_id, &t->ref_allele, &t->major_allele, &t->minor_allele,
                         &t->locus_type, &t->site_type, &t->gene_ids, &t->matrix_ids, nullptr};
  for (int k = 0; k < 9; ++k) {
    out25[2 * k] = s[k]->pool.data();
    out25[2 * k + 1] = s[k]->off.data();
    sizes10[k] = (int64_t)s[k]->pool.size();
  }
  sizes10[9] = 0;
  out25[18] = t->mean_coverage.data();
  out25[19] = t->fraction_covered.data();
  out25[20] = t->gene.data();
  out25[21] = t->freq.base ? t->freq.base + t->freq.body : nullptr;
  out25[22] = t->depth.base ? t->depth.base + t->depth.body : nullptr;
  out25[23] = nullptr;
  out25[24] = nullptr;
  return MIDAS_SNPS_OK;
}

int32_t midas_sites_tables_positions(midas_sites_tables* t, const void** out4, int64_t* sizes2, char* err1024) {
  if (!t || !out4 || !sizes2) return MIDAS_SNPS_ERR_INVALID_ARG;
  if (err1024) err1024[0] = 0;
  if (!t->have_positions) {
    const int32_t st = read_positions(t->dir + "/snps_info.txt", t, err1024);
    if (st != MIDAS_SNPS_OK) return st;
  }
  out4[0] = t->contig.data();
  out4[1] = t->ref_pos.data();
  out4[2] = t->contig_names.pool.data();
  out4[3] = t->contig_names.off.data();
  sizes2[0] = (int64_t)t->contig_names.off.size() - 1;
  sizes2[1] = (int64_t)t->contig_names.pool.size();
  return MIDAS_SNPS_OK;
}

void midas_sites_tables_close(midas_sites_tables* t) { delete t; }

int32_t midas_sites_parse_cell(int32_t kind, const char* text, int64_t n, void* out8) {
  if (!text || n < 0 || !out8) return MIDAS_SNPS_ERR_INVALID_ARG;
  const std::string_view v(text, (size_t)n);
  const bool ok = kind == 0 ? midas::parse_f64_py(v, static_cast<double*>(out8)) : midas::parse_i64_py(v, static_cast<int64_t*>(out8));
  return ok ? MIDAS_SNPS_OK : MIDAS_SNPS_ERR_BAD_LAYOUT;
}


// strain_tracking.py id_markers: site_id, allele, count_samples, count_A, count_T, count_C, count_G per marker
int32_t midas_sites_write_markers(const char* path, const midas_sites_tables* t, int64_t n_markers, const int32_t* rows7, char* err1024) {
  if (!path || !t || n_markers < 0 || (n_markers > 0 && !rows7)) return MIDAS_SNPS_ERR_INVALID_ARG;
  if (err1024) err1024[0] = 0;
  const int64_t n_sites = (int64_t)t->site_id.off.size() - 1;
  for (int64_t k = 0; k < n_markers; ++k)
    if (rows7[7 * k] < 0 || rows7[7 * k] >= n_sites || rows7[7 * k + 1] < 0 || rows7[7 * k + 1] > 3) {
      fail(err1024, path, 0, "a marker row names a site or an allele that does not exist");
      return MIDAS_SNPS_ERR_INVALID_ARG;
    }
  TextOut out;
  if (!out.open(path)) { fail(err1024, path, 0, "cannot be written"); return MIDAS_SNPS_ERR_INVALID_ARG; }
  out.put("site_id\tallele\tcount_samples\tcount_A\tcount_T\tcount_C\tcount_G\n");
  for (int64_t k = 0; k < n_markers; ++k) {
    const int32_t* r = rows7 + 7 * k;
    out.put(t->site_id.at((size_t)r[0]));
    out.put('\t');
    out.put("ATCG"[r[1]]);
    for (int c = 2; c < 7; ++c) { out.put('\t'); out.put_int(r[c]); }
    out.put('\n');
  }
  if (!out.close()) { fail(err1024, path, 0, "cannot be written"); return MIDAS_SNPS_ERR_INVALID_ARG; }
  return MIDAS_SNPS_OK;
}

// strain_tracking.py track_markers: sample1, sample2, count1, count2, count_both, count_either for every pair i < j
int32_t midas_sites_write_pairs(const char* path, const midas_sites_tables* t, int32_t n_samples, const int32_t* sample_row,
                                const int64_t* both, char* err1024) {
  if (!path || !t || n_samples < 1 || !sample_row || !both) return MIDAS_SNPS_ERR_INVALID_ARG;
  if (err1024) err1024[0] = 0;
  const int64_t n_rows = (int64_t)t->sample_ids.off.size() - 1;
  for (int32_t s = 0; s < n_samples; ++s)
    if (sample_row[s] < 0 || sample_row[s] >= n_rows) {
      fail(err1024, path, 0, "a sample names a row of snps_summary.txt that does not exist");
      return MIDAS_SNPS_ERR_INVALID_ARG;
    }
  TextOut out;
  if (!out.open(path)) { fail(err1024, path, 0, "cannot be written"); return MIDAS_SNPS_ERR_INVALID_ARG; }
  out.put("sample1\tsample2\tcount1\tcount2\tcount_both\tcount_either\n");
  const int64_t S = n_samples;
  for (int64_t i = 0; i < S; ++i)
    for (int64_t j = i + 1; j < S; ++j) {
      const int64_t c1 = both[i * S + i], c2 = both[j * S + j], b = both[i * S + j];
      out.put(t->sample_ids.at((size_t)sample_row[i]));
      out.put('\t');
      out.put(t->sample_ids.at((size_t)sample_row[j]));
      const int64_t v[4] = {c1, c2, b, c1 + c2 - b};
      for (int c = 0; c < 4; ++c) { out.put('\t'); out.put_int(v[c]); }
      out.put('\n');
    }
  if (!out.close()) { fail(err1024, path, 0, "cannot be written"); return MIDAS_SNPS_ERR_INVALID_ARG; }
  return MIDAS_SNPS_OK;
}

}  // extern "C"
