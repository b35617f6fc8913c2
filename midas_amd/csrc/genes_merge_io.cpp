// `merge_midas.py genes` on the host side: the readers and writers around the device merge (genes_merge.hip).
//
//   cluster map  DB/pan_genomes/<sp>/gene_info.txt[.gz] -> centroid_99 -> centroid_<pid> (read_cluster_map,
//                /root/reference/midas/merge/genes.py:91-98); the distinct clusters get indices in sorted byte order, so the
//                output's row order (sorted(), genes.py:40) is index order;
//   tables       the samples' genes/output/<sp>.genes.gz (build_gene_matrices' parse, genes.py:18-26): per sample the kept
//                rows' gene ids and the copy / depth / reads columns, one worker per file;
//   resolve      every row's gene id -> cluster index; a table whose ids are byte-equal to an earlier table's takes its
//                cluster vector as it is (tables of one species list the same genes in the same order);
//   matrices     genes_{presabs,copynum,depth,reads}.txt (write_gene_matrices, genes.py:32-48), str() of every cell.
//
// Both readers follow utility.parse_file (midas/utility.py:208-216) under Python 3: the file is read in universal-newline
// mode (\n, \r\n and a lone \r end a line), the header and every line are split on '\t', and a row whose field count
// differs from the header's is skipped.  A field is the value of the LAST header column of its name (dict(zip(...))).
// Numbers: float() / int() of the field after trimming ASCII whitespace; plain decimals and the nan / inf / infinity
// spellings only (Python would also take '1_0': a documented limit of this build, reported as an error).
#include <algorithm>
#include <atomic>
#include <charconv>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <string_view>
#include <thread>
#include <unordered_map>
#include <vector>

#include <zlib.h>

#include "../../include/midas_snps.h"
#include "text_numbers.h"
#include "workers.h"

namespace {

void set_err(char* err1024, const char* fmt, const std::string& a, const std::string& b = std::string(), long long n = -1) {
  if (!err1024) return;
  char line[32] = "";
  if (n >= 0) snprintf(line, sizeof line, "%lld", n);
  snprintf(err1024, 1024, fmt, a.c_str(), b.c_str(), line);
}

// the whole file, through zlib's gz layer (a plain file passes through)
bool slurp(const char* path, std::string* out) {
  gzFile f = gzopen(path, "rb");
  if (!f) return false;
  gzbuffer(f, 1 << 20);
  out->clear();
  std::vector<char> buf((size_t)1 << 22);
  for (;;) {
    const int n = gzread(f, buf.data(), (unsigned)buf.size());
    if (n < 0) { gzclose(f); return false; }
    if (n == 0) break;
    out->append(buf.data(), (size_t)n);
  }
  gzclose(f);
  return true;
}

// one line of the universal-newline view: [b, e) without its terminator; returns where the next line starts
size_t next_line(const std::string& s, size_t p, size_t* e) {
  const size_t n = s.size();
  size_t q = p;
  while (q < n && s[q] != '\n' && s[q] != '\r') ++q;
  *e = q;
  if (q < n && s[q] == '\r' && q + 1 < n && s[q + 1] == '\n') return q + 2;
  return q < n ? q + 1 : n;
}

void split_tabs(const char* b, const char* e, std::vector<std::string_view>* f) {
  f->clear();
  const char* p = b;
  for (const char* q = b;; ++q) {
    if (q == e || *q == '\t') {
      f->emplace_back(p, (size_t)(q - p));
      if (q == e) break;
      p = q + 1;
    }
  }
}

int last_column(const std::vector<std::string_view>& header, const char* name) {
  for (int k = (int)header.size() - 1; k >= 0; --k)
    if (header[k] == name) return k;
  return -1;
}

using midas::parse_f64;
using midas::parse_i64;

template <class F>
void for_each_index(int64_t n, int threads, F&& fn) {
  int nt = threads > 0 ? threads : midas::cpu_budget();
  nt = (int)std::max<int64_t>(1, std::min<int64_t>(nt, n));
  if (nt == 1) { for (int64_t i = 0; i < n; ++i) fn(i); return; }
  std::atomic<int64_t> next{0};
  std::vector<std::thread> th;
  for (int t = 0; t < nt; ++t)
    th.emplace_back([&] { for (int64_t i; (i = next.fetch_add(1)) < n;) fn(i); });
  for (auto& x : th) x.join();
}

}  // namespace

struct midas_genes_merge_map {
  std::string path;
  std::string cluster_ids;                 // the distinct clusters in sorted byte order, back to back
  std::vector<int64_t> cluster_off;        // n_clusters + 1
  std::string gene_ids;                    // the distinct centroid_99 ids, first appearance order
  std::vector<int64_t> gene_off;
  std::vector<uint32_t> gene_cluster;      // the cluster index the last row of the id gave it
  std::unordered_map<std::string_view, uint32_t> index;   // centroid_99 -> cluster index (views into gene_ids)
};

struct midas_genes_merge_tables {
  struct Table {
    std::string path;
    std::string ids;                       // the kept rows' gene ids back to back
    std::vector<int64_t> id_off;           // rows + 1
    std::vector<double> copy, depth;
    std::vector<int64_t> reads;
    std::vector<int64_t> skips;            // kept-row index at which each skipped line (wrong field count) stood
    std::vector<uint32_t> cluster;         // after resolve (empty when it shares another table's)
    int32_t same_as = -1;                  // the earlier table whose cluster vector this one uses, or -1
    int64_t rows() const { return (int64_t)id_off.size() - 1; }
    int64_t line_of(int64_t row) const {   // 1-based line of kept row `row` (the header is line 1)
      const int64_t before = (int64_t)(std::upper_bound(skips.begin(), skips.end(), row) - skips.begin());
      return row + 2 + before;
    }
  };
  std::vector<Table> t;
  const uint32_t* clusters_of(int32_t s) const {
    const Table& x = t[(size_t)s];
    return x.same_as >= 0 ? t[(size_t)x.same_as].cluster.data() : x.cluster.data();
  }
};

namespace {

int32_t read_table(const char* path, midas_genes_merge_tables::Table* tb, char* err1024) {
  tb->path = path;
  std::string text;
  if (!slurp(path, &text)) {
    set_err(err1024, "cannot read %s", path);
    return MIDAS_SNPS_ERR_INVALID_ARG;
  }
  size_t e = 0;
  size_t p = next_line(text, 0, &e);
  if (text.empty()) {
    set_err(err1024, "%s is empty: no header line", path);
    return MIDAS_SNPS_ERR_BAD_LAYOUT;
  }
  std::vector<std::string_view> header, f;
  split_tabs(text.data(), text.data() + e, &header);
  const int c_gene = last_column(header, "ref_id") >= 0 ? last_column(header, "ref_id") : last_column(header, "gene_id");
  const int c_copy = last_column(header, "normalized_coverage") >= 0 ? last_column(header, "normalized_coverage")
                                                                      : last_column(header, "copy_number");
  const int c_depth = last_column(header, "raw_coverage") >= 0 ? last_column(header, "raw_coverage") : last_column(header, "coverage");
  const int c_reads = last_column(header, "count_reads");
  tb->id_off.assign(1, 0);
  const size_t guess = text.size() / 48 + 1;
  tb->copy.reserve(guess); tb->depth.reserve(guess); tb->reads.reserve(guess); tb->id_off.reserve(guess + 1);
  int64_t line = 1;
  while (p < text.size()) {
    const size_t b = p;
    p = next_line(text, p, &e);
    ++line;
    split_tabs(text.data() + b, text.data() + e, &f);
    if (f.size() != header.size()) {
      tb->skips.push_back(tb->rows());
      continue;
    }
    const char* missing = c_gene < 0 ? "gene_id" : c_copy < 0 ? "copy_number" : c_depth < 0 ? "coverage" : nullptr;
    if (missing) {
      set_err(err1024, "%s: no '%s' column (line %s)", path, missing, line);
      return MIDAS_SNPS_ERR_BAD_LAYOUT;
    }
    double c = 0.0, d = 0.0;
    int64_t r = 0;
    if (!parse_f64(f[(size_t)c_copy], &c) || !parse_f64(f[(size_t)c_depth], &d)) {
      set_err(err1024, "%s%s, line %s: a coverage field is not a number this build reads", path, std::string(), line);
      return MIDAS_SNPS_ERR_BAD_LAYOUT;
    }
    if (c_reads >= 0 && !parse_i64(f[(size_t)c_reads], &r)) {
      set_err(err1024, "%s%s, line %s: count_reads is not a 64-bit decimal integer", path, std::string(), line);
      return MIDAS_SNPS_ERR_BAD_LAYOUT;
    }
    tb->ids.append(f[(size_t)c_gene].data(), f[(size_t)c_gene].size());
    tb->id_off.push_back((int64_t)tb->ids.size());
    tb->copy.push_back(c);
    tb->depth.push_back(d);
    tb->reads.push_back(r);
  }
  return MIDAS_SNPS_OK;
}

bool same_keys(const midas_genes_merge_tables::Table& a, const midas_genes_merge_tables::Table& b) {
  return a.id_off.size() == b.id_off.size() && a.ids.size() == b.ids.size() &&
         memcmp(a.ids.data(), b.ids.data(), a.ids.size()) == 0 &&
         memcmp(a.id_off.data(), b.id_off.data(), a.id_off.size() * sizeof(int64_t)) == 0;
}

// Python's repr() of a float: the shortest round-trip digits; fixed notation for decimal exponents in [-4, 16), with a
// fractional part always, otherwise d[.ddd]e(+|-)XX.  Returns the length written to out (<= 32).
int repr_f64(double v, char* out) {
  if (std::isnan(v)) { memcpy(out, "nan", 3); return 3; }
  if (std::isinf(v)) {
    if (v < 0) { memcpy(out, "-inf", 4); return 4; }
    memcpy(out, "inf", 3);
    return 3;
  }
  char sci[40];
  const auto r = std::to_chars(sci, sci + sizeof sci, v, std::chars_format::scientific);
  // sci = [-]d[.ddd]e(+|-)XX[X]
  const char* p = sci;
  char* o = out;
  if (*p == '-') *o++ = *p++;
  char digits[24];
  int nd = 0;
  for (; p < r.ptr && *p != 'e'; ++p)
    if (*p != '.') digits[nd++] = *p;
  int exp10 = 0;
  std::from_chars(p + 1 + (p[1] == '+'), r.ptr, exp10);
  if (exp10 < -4 || exp10 >= 16) {
    *o++ = digits[0];
    if (nd > 1) {
      *o++ = '.';
      memcpy(o, digits + 1, (size_t)(nd - 1));
      o += nd - 1;
    }
    *o++ = 'e';
    *o++ = exp10 < 0 ? '-' : '+';
    const int a = exp10 < 0 ? -exp10 : exp10;
    if (a >= 100) *o++ = (char)('0' + a / 100);
    *o++ = (char)('0' + a / 10 % 10);
    *o++ = (char)('0' + a % 10);
    return (int)(o - out);
  }
  if (exp10 < 0) {            // 0.000ddd
    *o++ = '0';
    *o++ = '.';
    for (int k = 0; k < -exp10 - 1; ++k) *o++ = '0';
    memcpy(o, digits, (size_t)nd);
    o += nd;
    return (int)(o - out);
  }
  const int ip = exp10 + 1;   // digits before the point
  for (int k = 0; k < ip; ++k) *o++ = k < nd ? digits[k] : '0';
  *o++ = '.';
  if (nd > ip) {
    memcpy(o, digits + ip, (size_t)(nd - ip));
    o += nd - ip;
  } else {
    *o++ = '0';
  }
  return (int)(o - out);
}

int i64_text(int64_t v, char* out) { return (int)(std::to_chars(out, out + 24, v).ptr - out); }

}  // namespace

extern "C" {

int32_t midas_genes_merge_map_open(const char* path, const char* cluster_column, midas_genes_merge_map** out, char* err1024) {
  if (!path || !cluster_column || !out) return MIDAS_SNPS_ERR_INVALID_ARG;
  *out = nullptr;
  std::string text;
  if (!slurp(path, &text)) {
    set_err(err1024, "cannot read the cluster map %s", path);
    return MIDAS_SNPS_ERR_INVALID_ARG;
  }
  if (text.empty()) {
    set_err(err1024, "%s is empty: no header line", path);
    return MIDAS_SNPS_ERR_BAD_LAYOUT;
  }
  auto* m = new midas_genes_merge_map();
  m->path = path;
  size_t e = 0;
  size_t p = next_line(text, 0, &e);
  std::vector<std::string_view> header, f;
  split_tabs(text.data(), text.data() + e, &header);
  const int c99 = last_column(header, "centroid_99"), cp = last_column(header, cluster_column);
  // pass 1: centroid_99 -> its last row's cluster id (a view into the text)
  std::unordered_map<std::string_view, std::string_view> last;
  std::vector<std::string_view> order;
  int64_t line = 1;
  while (p < text.size()) {
    const size_t b = p;
    p = next_line(text, p, &e);
    ++line;
    split_tabs(text.data() + b, text.data() + e, &f);
    if (f.size() != header.size()) continue;
    if (c99 < 0 || cp < 0) {
      set_err(err1024, "%s: no '%s' column (line %s)", path, c99 < 0 ? "centroid_99" : cluster_column, line);
      delete m;
      return MIDAS_SNPS_ERR_BAD_LAYOUT;
    }
    auto it = last.find(f[(size_t)c99]);
    if (it == last.end()) {
      last.emplace(f[(size_t)c99], f[(size_t)cp]);
      order.push_back(f[(size_t)c99]);
    } else {
      it->second = f[(size_t)cp];
    }
  }
  // the distinct clusters, sorted by bytes
  std::vector<std::string_view> cl;
  cl.reserve(last.size());
  for (const auto& kv : last) cl.push_back(kv.second);
  std::sort(cl.begin(), cl.end());
  cl.erase(std::unique(cl.begin(), cl.end()), cl.end());
  std::unordered_map<std::string_view, uint32_t> cidx;
  cidx.reserve(cl.size());
  m->cluster_off.assign(1, 0);
  for (size_t k = 0; k < cl.size(); ++k) {
    cidx.emplace(cl[k], (uint32_t)k);
    m->cluster_ids.append(cl[k].data(), cl[k].size());
    m->cluster_off.push_back((int64_t)m->cluster_ids.size());
  }
  m->gene_off.assign(1, 0);
  size_t gbytes = 0;
  for (const auto& g : order) gbytes += g.size();
  m->gene_ids.reserve(gbytes);
  for (const auto& g : order) {
    m->gene_ids.append(g.data(), g.size());
    m->gene_off.push_back((int64_t)m->gene_ids.size());
    m->gene_cluster.push_back(cidx[last[g]]);
  }
  m->index.reserve(order.size());
  for (size_t k = 0; k < order.size(); ++k)
    m->index.emplace(std::string_view(m->gene_ids.data() + m->gene_off[k], (size_t)(m->gene_off[k + 1] - m->gene_off[k])),
                     m->gene_cluster[k]);
  *out = m;
  return MIDAS_SNPS_OK;
}

int64_t midas_genes_merge_map_n_clusters(const midas_genes_merge_map* m) { return m ? (int64_t)m->cluster_off.size() - 1 : -1; }

int64_t midas_genes_merge_map_n_genes(const midas_genes_merge_map* m) { return m ? (int64_t)m->gene_cluster.size() : -1; }

int32_t midas_genes_merge_map_columns(const midas_genes_merge_map* m, const void** out5, int64_t* sizes2) {
  if (!m || !out5 || !sizes2) return MIDAS_SNPS_ERR_INVALID_ARG;
  out5[0] = m->cluster_ids.data();
  out5[1] = m->cluster_off.data();
  out5[2] = m->gene_ids.data();
  out5[3] = m->gene_off.data();
  out5[4] = m->gene_cluster.data();
  sizes2[0] = (int64_t)m->cluster_ids.size();
  sizes2[1] = (int64_t)m->gene_ids.size();
  return MIDAS_SNPS_OK;
}

void midas_genes_merge_map_close(midas_genes_merge_map* m) { delete m; }

int32_t midas_genes_merge_tables_open(int32_t n_tables, const char* const* paths, int32_t threads, midas_genes_merge_tables** out,
                                      char* err1024) {
  if (n_tables < 0 || (n_tables > 0 && !paths) || !out) return MIDAS_SNPS_ERR_INVALID_ARG;
  *out = nullptr;
  auto* ts = new midas_genes_merge_tables();
  ts->t.resize((size_t)n_tables);
  std::vector<int32_t> st((size_t)n_tables, MIDAS_SNPS_OK);
  std::vector<std::string> msg((size_t)n_tables);
  for_each_index(n_tables, threads, [&](int64_t i) {
    char e[1024] = "";
    st[(size_t)i] = read_table(paths[i], &ts->t[(size_t)i], e);
    msg[(size_t)i] = e;
  });
  for (int32_t i = 0; i < n_tables; ++i)       // the first sample in input order decides, as the reference's loop would
    if (st[(size_t)i] != MIDAS_SNPS_OK) {
      if (err1024) snprintf(err1024, 1024, "%s", msg[(size_t)i].c_str());
      delete ts;
      return st[(size_t)i];
    }
  *out = ts;
  return MIDAS_SNPS_OK;
}

int64_t midas_genes_merge_tables_rows(const midas_genes_merge_tables* ts, int32_t table) {
  if (!ts || table < 0 || (size_t)table >= ts->t.size()) return -1;
  return ts->t[(size_t)table].rows();
}

int32_t midas_genes_merge_tables_columns(const midas_genes_merge_tables* ts, int32_t table, const void** out6, int64_t* out_id_bytes,
                                         int32_t* out_same_as) {
  if (!ts || table < 0 || (size_t)table >= ts->t.size() || !out6) return MIDAS_SNPS_ERR_INVALID_ARG;
  const auto& x = ts->t[(size_t)table];
  out6[0] = x.ids.data();
  out6[1] = x.id_off.data();
  out6[2] = x.copy.data();
  out6[3] = x.depth.data();
  out6[4] = x.reads.data();
  out6[5] = ts->clusters_of(table);
  if (out_id_bytes) *out_id_bytes = (int64_t)x.ids.size();
  if (out_same_as) *out_same_as = x.same_as;
  return MIDAS_SNPS_OK;
}

int32_t midas_genes_merge_tables_resolve(midas_genes_merge_tables* ts, const midas_genes_merge_map* m, int32_t reuse, int32_t threads,
                                         char* err1024) {
  if (!ts || !m) return MIDAS_SNPS_ERR_INVALID_ARG;
  const int32_t n = (int32_t)ts->t.size();
  std::vector<int32_t> own;        // the tables that look their ids up
  for (int32_t s = 0; s < n; ++s) {
    auto& x = ts->t[(size_t)s];
    x.same_as = -1;
    x.cluster.clear();
    if (reuse)
      for (int32_t r : own)
        if (same_keys(ts->t[(size_t)r], x)) { x.same_as = r; break; }
    if (x.same_as < 0) own.push_back(s);
  }
  std::vector<int64_t> bad((size_t)n, -1);
  for_each_index((int64_t)own.size(), threads, [&](int64_t k) {
    auto& x = ts->t[(size_t)own[(size_t)k]];
    const int64_t rows = x.rows();
    x.cluster.resize((size_t)rows);
    for (int64_t i = 0; i < rows; ++i) {
      const auto it = m->index.find(std::string_view(x.ids.data() + x.id_off[(size_t)i], (size_t)(x.id_off[(size_t)i + 1] - x.id_off[(size_t)i])));
      if (it == m->index.end()) { bad[(size_t)own[(size_t)k]] = i; return; }
      x.cluster[(size_t)i] = it->second;
    }
  });
  for (int32_t s = 0; s < n; ++s)
    if (bad[(size_t)s] >= 0) {
      const auto& x = ts->t[(size_t)s];
      const int64_t i = bad[(size_t)s];
      const std::string id(x.ids.data() + x.id_off[(size_t)i], (size_t)(x.id_off[(size_t)i + 1] - x.id_off[(size_t)i]));
      if (err1024)
        snprintf(err1024, 1024, "gene '%.200s' of %.350s (line %lld) is not in the cluster map %.350s", id.c_str(), x.path.c_str(),
                 (long long)x.line_of(i), m->path.c_str());
      return MIDAS_SNPS_ERR_BAD_LAYOUT;
    }
  return MIDAS_SNPS_OK;
}

void midas_genes_merge_tables_close(midas_genes_merge_tables* ts) { delete ts; }

int32_t midas_genes_merge_format_f64(int64_t n, const double* v, char* out, int64_t capacity, int64_t* out_len) {
  if (n < 0 || (n > 0 && !v) || !out || !out_len || capacity < 33 * n) return MIDAS_SNPS_ERR_INVALID_ARG;
  char* o = out;
  for (int64_t i = 0; i < n; ++i) {
    o += repr_f64(v[i], o);
    *o++ = '\n';
  }
  *out_len = (int64_t)(o - out);
  return MIDAS_SNPS_OK;
}

int32_t midas_genes_merge_write_matrix(const char* path, const char* header_line, int32_t kind, int64_t n_rows, const uint32_t* row_cluster,
                                       const char* cluster_ids, const int64_t* cluster_off, int32_t n_samples, const void* values,
                                       const uint8_t* state, int32_t threads, char* err1024) {
  if (!path || !header_line || kind < 0 || kind > 2 || n_rows < 0 || n_samples < 0 ||
      (n_rows > 0 && (!row_cluster || !cluster_ids || !cluster_off || (n_samples > 0 && (kind == 0 ? !state : !values)))))
    return MIDAS_SNPS_ERR_INVALID_ARG;
  FILE* f = fopen(path, "wb");
  if (!f) {
    set_err(err1024, "cannot write %s", path);
    return MIDAS_SNPS_ERR_INVALID_ARG;
  }
  bool ok = fputs(header_line, f) >= 0;
  // row blocks formatted in parallel, written in order
  const int64_t block = 4096;
  const int64_t n_blocks = (n_rows + block - 1) / block;
  const int nt = std::max(1, threads > 0 ? threads : midas::cpu_budget());
  const int64_t wave = (int64_t)nt * 4;
  std::vector<std::string> text;
  const double* vf = static_cast<const double*>(values);
  const int64_t* vi = static_cast<const int64_t*>(values);
  for (int64_t b0 = 0; b0 < n_blocks && ok; b0 += wave) {
    const int64_t nb = std::min(wave, n_blocks - b0);
    text.assign((size_t)nb, std::string());
    for_each_index(nb, nt, [&](int64_t k) {
      std::string& s = text[(size_t)k];
      const int64_t r0 = (b0 + k) * block, r1 = std::min(n_rows, r0 + block);
      s.reserve((size_t)((r1 - r0) * (24 + 12 * (int64_t)n_samples)));
      char cell[40];
      for (int64_t r = r0; r < r1; ++r) {
        const uint32_t c = row_cluster[r];
        s.append(cluster_ids + cluster_off[c], (size_t)(cluster_off[c + 1] - cluster_off[c]));
        const int64_t base = r * (int64_t)n_samples;
        for (int32_t j = 0; j < n_samples; ++j) {
          cell[0] = '\t';
          int len;
          if (kind == 0) {
            const uint8_t st = state[base + j];
            if (st == 0) { memcpy(cell + 1, "0.0", 3); len = 3; }
            else { cell[1] = st == 2 ? '1' : '0'; len = 1; }
          } else if (kind == 1) {
            len = repr_f64(vf[base + j], cell + 1);
          } else {
            len = i64_text(vi[base + j], cell + 1);
          }
          s.append(cell, (size_t)len + 1);
        }
        s.push_back('\n');
      }
    });
    for (const auto& s : text)
      if (fwrite(s.data(), 1, s.size(), f) != s.size()) { ok = false; break; }
  }
  if (fclose(f) != 0) ok = false;
  if (!ok) {
    set_err(err1024, "write failed: %s", path);
    return MIDAS_SNPS_ERR_INVALID_ARG;
  }
  return MIDAS_SNPS_OK;
}

}  // extern "C"
