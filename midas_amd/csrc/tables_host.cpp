// The <species>.snps.gz tables on the host: their readers, the row / matrix / info writers and the gzip members they are made of.
#include "hostio_internal.h"
#include "tables_plan.h"

// One sample's <species>.snps.gz, parsed: what build_temp_count_matrix (midas/merge/snps.py:246-271) extracts.
struct ParsedRows {
  std::vector<uint32_t> counts;   // 4 per row: r[-4:]
  std::string keys;               // 'ref_id|ref_pos|ref_allele' back to back
  std::vector<int64_t> key_end;   // per row, end offset within `keys`
  int64_t rows = 0;
  int64_t bad_row = -1;           // first malformed row of the piece (0-based within the piece), or -1
};

struct midas_snps_table {
  // the table as parsed pieces (parallel parse), plus where each piece lands in the caller's arrays
  std::vector<ParsedRows> pieces;
  std::vector<int64_t> skip;       // rows of each piece in front of the wanted range
  std::vector<int64_t> take;       // rows used of each piece (the range may cut the first and the last one)
  std::vector<int64_t> row_base;   // first row of each piece
  std::vector<int64_t> key_base;   // first key byte of each piece
  int64_t rows = 0, key_bytes = 0;
};

struct TableSetMember { size_t data, clen, ulen; int64_t row0, rows; };   // row0: table row of the member's first row
struct midas_snps_tableset {
  std::vector<std::string> paths;
  std::vector<RawBuf<uint8_t>> files;
  std::vector<std::vector<TableSetMember>> members;    // per table, the members that hold rows
  std::vector<std::vector<midas::TableMemberSpan>> all; // per table that announces its rows, every member in file order (the device readers plan over them)
  std::vector<int64_t> rows;                            // per table, -1 = the file does not announce its rows
};

namespace {

// One gzip member around a raw deflate stream.  The header carries an extra subfield 'M','S' with the member's
// total size in bytes (the BGZF idea): any gzip reader skips it, ours uses it to find the members of a table without
// inflating them, so that members are inflated and parsed in parallel (midas_snps_table_open).
constexpr size_t kGzHeaderOld = 20;   // round-1 files: 10 fixed + XLEN(2) + 'M','S',len(2) + u32
constexpr size_t kGzHeader = 28;      // + 'M','R',len(2) + u32: the member's table rows (a rank of a sharded merge reads
                                      // only the members that hold its row range)
// `out` is sized to the member; the deflate runs into a scratch buffer the calling thread keeps (sizing `out` to
// deflateBound first would zero-fill and page-fault as many bytes as the text itself, once per member).
bool gz_member(const uint8_t* in, size_t n, int level, std::vector<uint8_t>& result, uint32_t rows = 0) {
  z_stream zs;
  memset(&zs, 0, sizeof zs);
  if (deflateInit2(&zs, level, Z_DEFLATED, -15, 8, Z_DEFAULT_STRATEGY) != Z_OK) return false;
  static thread_local std::vector<uint8_t> out;
  const size_t cap = kGzHeader + deflateBound(&zs, (uLong)n) + 64;
  if (out.size() < cap) out.resize(cap);
  zs.next_in = const_cast<Bytef*>(in);
  zs.avail_in = (uInt)n;
  zs.next_out = out.data() + kGzHeader;
  zs.avail_out = (uInt)(out.size() - kGzHeader - 8);
  const int rc = deflate(&zs, Z_FINISH);
  const size_t produced = (out.size() - kGzHeader - 8) - zs.avail_out;
  deflateEnd(&zs);
  if (rc != Z_STREAM_END) return false;
  const size_t total = kGzHeader + produced + 8;
  if (total > 0xFFFFFFFFull) return false;
  static const uint8_t fixed[10] = {0x1f, 0x8b, 8, 4 /* FEXTRA */, 0, 0, 0, 0, 0, 255};
  memcpy(out.data(), fixed, 10);
  const uint8_t extra[18] = {16, 0, 'M', 'S', 4, 0, (uint8_t)total, (uint8_t)(total >> 8), (uint8_t)(total >> 16),
                             (uint8_t)(total >> 24), 'M', 'R', 4, 0, (uint8_t)rows, (uint8_t)(rows >> 8),
                             (uint8_t)(rows >> 16), (uint8_t)(rows >> 24)};
  memcpy(out.data() + 10, extra, 18);
  const uint32_t crc = (uint32_t)crc32(crc32(0L, Z_NULL, 0), in, (uInt)n);
  const uint32_t isize = (uint32_t)n;
  memcpy(out.data() + kGzHeader + produced, &crc, 4);
  memcpy(out.data() + kGzHeader + produced + 4, &isize, 4);
  result.assign(out.begin(), out.begin() + (ptrdiff_t)total);
  return true;
}

// The same member around the row coder's stream (row_deflate.h): for table rows, whose structure the formatter knows.
bool gz_member_rows(const uint8_t* in, size_t n, const uint32_t* row_begin, const uint32_t* tail_begin, size_t n_rows,
                    std::vector<uint8_t>& result, uint32_t rows) {
  static thread_local midas::RowDeflate coder;
  static thread_local std::vector<uint8_t> out;
  out.clear();
  out.resize(kGzHeader);
  coder.compress(in, n, row_begin, tail_begin, n_rows, out);
  const size_t total = out.size() + 8;
  if (total > 0xFFFFFFFFull) return false;
  static const uint8_t fixed[10] = {0x1f, 0x8b, 8, 4 /* FEXTRA */, 0, 0, 0, 0, 0, 255};
  memcpy(out.data(), fixed, 10);
  const uint8_t extra[18] = {16, 0, 'M', 'S', 4, 0, (uint8_t)total, (uint8_t)(total >> 8), (uint8_t)(total >> 16),
                             (uint8_t)(total >> 24), 'M', 'R', 4, 0, (uint8_t)rows, (uint8_t)(rows >> 8),
                             (uint8_t)(rows >> 16), (uint8_t)(rows >> 24)};
  memcpy(out.data() + 10, extra, 18);
  const uint32_t crc = (uint32_t)crc32(crc32(0L, Z_NULL, 0), in, (uInt)n);
  const uint32_t isize = (uint32_t)n;
  uint8_t tail[8];
  memcpy(tail, &crc, 4);
  memcpy(tail + 4, &isize, 4);
  out.insert(out.end(), tail, tail + 8);
  result.assign(out.begin(), out.end());
  return true;
}

// fields: ref_id, ref_pos, ref_allele, depth, count_a, count_c, count_g, count_t (tab separated); the reference takes
// r[0:3] for the site key and r[-4:] for the counts (midas/merge/snps.py:262-270)
void parse_rows(const char* b, const char* end, bool want_keys, bool skip_first_line, ParsedRows& out) {
  if (skip_first_line) {
    const char* nl = (const char*)memchr(b, '\n', (size_t)(end - b));
    b = nl ? nl + 1 : end;
  }
  while (b < end) {
    const char* nl = (const char*)memchr(b, '\n', (size_t)(end - b));
    const char* e = nl ? nl : end;
    const char* tabs[16];
    int nt = 0;
    for (const char* q = b; q < e && nt < 16; ++q)
      if (*q == '\t') tabs[nt++] = q;
    bool ok = nt >= 7;
    uint32_t v4[4] = {0, 0, 0, 0};
    if (ok) {
      const char* starts[4] = {tabs[nt - 4] + 1, tabs[nt - 3] + 1, tabs[nt - 2] + 1, tabs[nt - 1] + 1};
      const char* ends[4] = {tabs[nt - 3], tabs[nt - 2], tabs[nt - 1], e};
      for (int k = 0; k < 4 && ok; ++k) {
        uint64_t v = 0;
        if (starts[k] >= ends[k]) ok = false;
        for (const char* q = starts[k]; q < ends[k] && ok; ++q) {
          if (*q < '0' || *q > '9') { ok = false; break; }
          v = v * 10 + (uint64_t)(*q - '0');
          if (v > 0x7FFFFFFFull) ok = false;   // major + minor of one sample must fit 32 bits downstream
        }
        v4[k] = (uint32_t)v;
      }
    }
    if (!ok) { out.bad_row = out.rows; return; }
    if (want_keys) {
      out.keys.append(b, tabs[0]);
      out.keys.push_back('|');
      out.keys.append(tabs[0] + 1, tabs[1]);
      out.keys.push_back('|');
      out.keys.append(tabs[1] + 1, tabs[2]);
      out.key_end.push_back((int64_t)out.keys.size());
    }
    out.counts.insert(out.counts.end(), v4, v4 + 4);
    ++out.rows;
    b = nl ? nl + 1 : end;
  }
}

}  // namespace

extern "C" {

namespace {
// The gzip members of a table written by this library, found without inflating anything: {data offset, compressed bytes,
// uncompressed bytes, table rows (-1: a round-1 file that does not say)}.  Empty when the file is any other gzip file.
struct TableMember { size_t data, clen, ulen; int64_t rows; };
std::vector<TableMember> table_members_of(const uint8_t* bytes, size_t n_bytes) {
  struct Span { const uint8_t* d; size_t n; size_t size() const { return n; } const uint8_t* data() const { return d; } } file{bytes, n_bytes};
  std::vector<TableMember> members;
  size_t p = 0;
  while (p < file.size()) {
    const uint8_t* h = file.data() + p;
    if (p + kGzHeaderOld + 8 > file.size() || h[0] != 0x1f || h[1] != 0x8b || h[2] != 8 || h[3] != 4 || h[12] != 'M' ||
        h[13] != 'S' || rd16(h + 14) != 4) return {};
    const size_t xlen = rd16(h + 10);
    int64_t rows = -1;
    if (xlen == 16 && p + kGzHeader + 8 <= file.size() && h[20] == 'M' && h[21] == 'R' && rd16(h + 22) == 4) rows = rd32(h + 24);
    else if (xlen != 8) return {};
    const size_t hdr = 12 + xlen, total = rd32(h + 16);
    if (total < hdr + 8 || p + total > file.size()) return {};
    members.push_back({p + hdr, total - hdr - 8, (size_t)rd32(h + total - 4), rows});
    p += total;
  }
  return members;
}

std::vector<TableMember> table_members(const std::vector<uint8_t>& file) { return table_members_of(file.data(), file.size()); }

bool read_file(const char* path, std::vector<uint8_t>& file, char* err256) {
  FILE* f = fopen(path, "rb");
  if (!f) { set_err(err256, "cannot open %s", path); return false; }
  fseek(f, 0, SEEK_END);
  const long fsz = ftell(f);
  fseek(f, 0, SEEK_SET);
  file.resize((size_t)(fsz > 0 ? fsz : 0));
  const bool rd = file.empty() || fread(file.data(), 1, file.size(), f) == file.size();
  fclose(f);
  if (!rd) set_err(err256, "short read on %s", path);
  return rd;
}
}  // namespace

int32_t midas_snps_table_count_rows(const char* path, int64_t* out_rows, char* err256) {
  if (!path || !out_rows) return MIDAS_SNPS_ERR_INVALID_ARG;
  *out_rows = -1;
  // only the gzip member headers are read (28 bytes each, found by the sizes the members announce): every rank of a merge
  // asks this of every sample's table before any work starts, and reading whole files for it was N full reads of all inputs
  const int fd = open(path, O_RDONLY);
  if (fd < 0) { set_err(err256, "cannot open %s", path); return MIDAS_SNPS_ERR_INVALID_ARG; }
  struct stat sb;
  if (fstat(fd, &sb) != 0) { close(fd); set_err(err256, "cannot stat %s", path); return MIDAS_SNPS_ERR_INVALID_ARG; }
  const uint64_t fsz = (uint64_t)sb.st_size;
  uint64_t p = 0;
  int64_t rows = 0;
  bool ours = fsz > 0;
  while (ours && p < fsz) {
    uint8_t h[kGzHeader];
    const size_t want = (size_t)std::min<uint64_t>(kGzHeader, fsz - p);
    if (want < (size_t)kGzHeaderOld || pread(fd, h, want, (off_t)p) != (ssize_t)want) { ours = false; break; }
    if (h[0] != 0x1f || h[1] != 0x8b || h[2] != 8 || h[3] != 4 || h[12] != 'M' || h[13] != 'S' || rd16(h + 14) != 4) { ours = false; break; }
    const size_t xlen = rd16(h + 10);
    if (!(xlen == 16 && want >= (size_t)kGzHeader && h[20] == 'M' && h[21] == 'R' && rd16(h + 22) == 4)) { ours = false; break; }   // (xlen 8: a round-1 file)
    const uint64_t total = rd32(h + 16);
    if (total < 12 + xlen + 8 || p + total > fsz) { ours = false; break; }
    rows += rd32(h + 24);
    p += total;
  }
  close(fd);
  if (ours) *out_rows = rows;      // else: not one of ours (or a file that does not say): unknown without reading it
  return MIDAS_SNPS_OK;
}

int32_t midas_snps_table_open_range(const char* path, int64_t row_begin, int64_t row_end, int32_t want_keys,
                                    midas_snps_table** out, char* err256) {
  if (!path || !out || row_begin < 0) return MIDAS_SNPS_ERR_INVALID_ARG;
  *out = nullptr;
  // ---- the text of the table, as line-aligned pieces ------------------------------------------------------
  std::vector<std::vector<char>> pieces;
  std::vector<ParsedRows> fused;       // members of one of our own files: inflated and parsed in one task each
  bool have_fused = false;
  std::vector<uint8_t> file;
  if (!read_file(path, file, err256)) return MIDAS_SNPS_ERR_INVALID_ARG;
  // members written by midas_snps_write_rows/_table/_part announce their size (and rows): walk them without inflating
  std::vector<TableMember> members = table_members(file);
  int64_t first_row = 0;           // table row of the first row that will be parsed
  size_t header_piece = 0;         // the piece whose first line is the header line (SIZE_MAX: not among the pieces)
  const int nt = hw_threads(0);
  if (!members.empty()) {
    bool counted = true;
    for (const TableMember& m : members) counted = counted && m.rows >= 0;
    if (counted) {                 // only the members that hold rows [row_begin, row_end)
      std::vector<TableMember> wanted;
      int64_t at = 0;
      bool first = true;
      header_piece = (size_t)-1;
      for (size_t i = 0; i < members.size(); ++i) {
        const int64_t lo = at, hi = at + members[i].rows;
        at = hi;
        if (members[i].rows == 0 || hi <= row_begin || (row_end >= 0 && lo >= row_end)) continue;
        if (first) { first_row = lo; first = false; }
        wanted.push_back(members[i]);
      }
      if (first) first_row = row_begin;
      members.swap(wanted);
    }
    // inflate and parse in one task per member: the text lives in a buffer the thread keeps (a vector per member would
    // be zero-filled and page-faulted once per member: as many bytes again as the text itself)
    size_t header_member = (size_t)-1;
    if (header_piece != (size_t)-1) {
      header_member = 0;
      while (header_member < members.size() && members[header_member].ulen == 0) ++header_member;
    }
    fused.resize(members.size());
    std::atomic<int> bad{0};
    run_pool(nt, members.size(), [&](size_t i) {
      static thread_local std::vector<char> text;
      const TableMember& m = members[i];
      if (m.ulen == 0) return;
      if (text.size() < m.ulen) text.resize(m.ulen);
      if (!raw_inflate(file.data() + m.data, (size_t)m.clen, reinterpret_cast<uint8_t*>(text.data()), (size_t)m.ulen)) { bad = 1; return; }
      ParsedRows& pr = fused[i];
      if (m.rows > 0) {
        pr.counts.reserve((size_t)m.rows * 4);
        if (want_keys) { pr.key_end.reserve((size_t)m.rows); pr.keys.reserve((size_t)m.rows * 24); }
      }
      parse_rows(text.data(), text.data() + m.ulen, want_keys != 0, i == header_member, pr);
    });
    if (bad) { set_err(err256, "%s: corrupt deflate data", path); return MIDAS_SNPS_ERR_BAD_LAYOUT; }
    have_fused = true;
  } else {
    // any other gzip file (e.g. written by the reference): one serial inflate, then line-aligned pieces
    std::vector<uint8_t>().swap(file);
    gzFile f = gzopen(path, "rb");   // transparently reads concatenated gzip members
    if (!f) { set_err(err256, "cannot open %s", path); return MIDAS_SNPS_ERR_INVALID_ARG; }
    gzbuffer(f, 1 << 20);
    const size_t kPiece = (size_t)4 << 20;
    std::vector<char> cur;
    cur.reserve(kPiece + (1 << 16));
    std::vector<char> buf(1 << 20);
    bool ok = true;
    for (;;) {
      const int n = gzread(f, buf.data(), (unsigned)buf.size());
      if (n < 0) { ok = false; break; }
      if (n == 0) break;
      cur.insert(cur.end(), buf.data(), buf.data() + n);
      if (cur.size() >= kPiece) {   // cut after the last complete line
        size_t cut = cur.size();
        while (cut > 0 && cur[cut - 1] != '\n') --cut;
        if (cut > 0) {
          std::vector<char> rest(cur.begin() + (long)cut, cur.end());
          cur.resize(cut);
          pieces.push_back(std::move(cur));
          cur = std::move(rest);
          cur.reserve(kPiece + (1 << 16));
        }
      }
    }
    gzclose(f);
    if (!ok) { set_err(err256, "%s: corrupt gzip data", path); return MIDAS_SNPS_ERR_BAD_LAYOUT; }
    if (!cur.empty()) pieces.push_back(std::move(cur));
  }
  std::vector<uint8_t>().swap(file);
  // ---- parse the pieces in parallel (the first line of the file is the header) --------------------------------
  if (header_piece != (size_t)-1) {
    header_piece = 0;
    while (header_piece < pieces.size() && pieces[header_piece].empty()) ++header_piece;
  }
  std::vector<ParsedRows> parsed;
  if (have_fused) {
    parsed.swap(fused);
  } else {
    parsed.resize(pieces.size());
    run_pool(nt, pieces.size(), [&](size_t i) {
      const std::vector<char>& t = pieces[i];
      if (t.empty()) return;
      parse_rows(t.data(), t.data() + t.size(), want_keys != 0, i == header_piece, parsed[i]);
      std::vector<char>().swap(pieces[i]);
    });
  }
  midas_snps_table* tab = new (std::nothrow) midas_snps_table();
  if (!tab) return MIDAS_SNPS_ERR_OUT_OF_MEMORY;
  tab->skip.assign(parsed.size(), 0);
  tab->take.assign(parsed.size(), 0);
  tab->row_base.assign(parsed.size(), 0);
  tab->key_base.assign(parsed.size(), 0);
  int64_t rows = 0, kbytes = 0, at = first_row;
  for (size_t i = 0; i < parsed.size(); ++i) {
    ParsedRows& pr = parsed[i];
    const int64_t lo = at, hi = at + pr.rows;     // table rows of this piece
    at = hi;
    const int64_t use_lo = std::max(lo, row_begin), use_hi = row_end >= 0 ? std::min(hi, row_end) : hi;
    if (pr.bad_row >= 0 && lo + pr.bad_row >= row_begin && (row_end < 0 || lo + pr.bad_row < row_end)) {
      // a malformed row inside what would be read (the reference would fail converting it)
      set_err(err256, "%s: malformed row %lld", path, (long long)(lo + pr.bad_row + 1));
      delete tab;
      return MIDAS_SNPS_ERR_BAD_LAYOUT;
    }
    if (use_hi <= use_lo) { if (row_end >= 0 && lo >= row_end) break; continue; }
    tab->skip[i] = use_lo - lo;
    tab->take[i] = use_hi - use_lo;
    tab->row_base[i] = rows;
    tab->key_base[i] = kbytes;
    rows += use_hi - use_lo;
    if (want_keys) kbytes += pr.key_end[(size_t)(use_hi - lo) - 1] - (use_lo > lo ? pr.key_end[(size_t)(use_lo - lo) - 1] : 0);
  }
  tab->rows = rows;
  tab->key_bytes = kbytes;
  tab->pieces = std::move(parsed);
  *out = tab;
  return MIDAS_SNPS_OK;
}

int32_t midas_snps_tableset_open(int32_t n_tables, const char* const* paths, midas_snps_tableset** out, int64_t* rows_each,
                                 char* err256) {
  if (n_tables <= 0 || !paths || !out || !rows_each) return MIDAS_SNPS_ERR_INVALID_ARG;
  *out = nullptr;
  std::unique_ptr<midas_snps_tableset> ts(new (std::nothrow) midas_snps_tableset());
  if (!ts) return MIDAS_SNPS_ERR_OUT_OF_MEMORY;
  const size_t n = (size_t)n_tables;
  ts->paths.resize(n);
  ts->files.resize(n);
  ts->members.resize(n);
  ts->all.resize(n);
  ts->rows.assign(n, -1);
  // every file in 8 MiB pieces, all pieces of all files in one parallel region
  struct Piece { size_t table, off, len; };
  std::vector<Piece> pieces;
  std::vector<int> fds(n, -1);
  int32_t st = MIDAS_SNPS_OK;
  for (size_t t = 0; t < n && st == MIDAS_SNPS_OK; ++t) {
    if (!paths[t]) { st = MIDAS_SNPS_ERR_INVALID_ARG; break; }
    ts->paths[t] = paths[t];
    fds[t] = open(paths[t], O_RDONLY);
    struct stat sb;
    if (fds[t] < 0 || fstat(fds[t], &sb) != 0) { set_err(err256, "cannot open %s", paths[t]); st = MIDAS_SNPS_ERR_INVALID_ARG; break; }
    if (!ts->files[t].resize((size_t)sb.st_size)) { set_err(err256, "out of memory reading %s", paths[t]); st = MIDAS_SNPS_ERR_OUT_OF_MEMORY; break; }
    for (size_t off = 0; off < (size_t)sb.st_size; off += (size_t)8 << 20)
      pieces.push_back({t, off, std::min((size_t)8 << 20, (size_t)sb.st_size - off)});
  }
  std::atomic<int> short_read{-1};
  if (st == MIDAS_SNPS_OK)
    run_pool(hw_threads(0), pieces.size(), [&](size_t k) {
      const Piece& pc = pieces[k];
      size_t done = 0;
      while (done < pc.len) {
        const ssize_t got = pread(fds[pc.table], ts->files[pc.table].data() + pc.off + done, pc.len - done, (off_t)(pc.off + done));
        if (got <= 0) { short_read = (int)pc.table; return; }
        done += (size_t)got;
      }
    });
  for (int fd : fds) if (fd >= 0) close(fd);
  if (st != MIDAS_SNPS_OK) return st;
  if (short_read >= 0) { set_err(err256, "short read on %s", paths[short_read.load()]); return MIDAS_SNPS_ERR_INVALID_ARG; }
  for (size_t t = 0; t < n; ++t) {
    const std::vector<TableMember> all = table_members_of(ts->files[t].data(), ts->files[t].size());
    bool counted = !all.empty();
    for (const TableMember& m : all) counted = counted && m.rows >= 0;
    if (!counted) continue;                      // written by the reference (or round 1): the caller reads it the other way
    int64_t at = 0;
    for (const TableMember& m : all) {
      if (m.rows > 0) ts->members[t].push_back({m.data, m.clen, m.ulen, at, m.rows});
      ts->all[t].push_back(midas::TableMemberSpan{(uint64_t)m.data, (uint32_t)m.clen, (uint32_t)m.ulen, m.rows});
      at += m.rows;
    }
    ts->rows[t] = at;
  }
  memcpy(rows_each, ts->rows.data(), n * sizeof(int64_t));
  *out = ts.release();
  return MIDAS_SNPS_OK;
}

void midas_snps_tableset_close(midas_snps_tableset* ts) { delete ts; }

}  // extern "C"
namespace midas {
// the open set as the device readers see it (hostio.h)
int32_t tableset_tables(const midas_snps_tableset* ts) { return (int32_t)ts->paths.size(); }
const char* tableset_path(const midas_snps_tableset* ts, int32_t t) { return ts->paths[(size_t)t].c_str(); }
const uint8_t* tableset_file(const midas_snps_tableset* ts, int32_t t, size_t* bytes) { *bytes = ts->files[(size_t)t].size(); return ts->files[(size_t)t].data(); }
int64_t tableset_rows(const midas_snps_tableset* ts, int32_t t) { return ts->rows[(size_t)t]; }
const std::vector<TableMemberSpan>& tableset_members(const midas_snps_tableset* ts, int32_t t) { return ts->all[(size_t)t]; }
}  // namespace midas
extern "C" {

int32_t midas_snps_tableset_read_counts(midas_snps_tableset* ts, int64_t row_begin, int64_t n_rows, uint32_t* const* out_counts,
                                        char* err256) {
  if (!ts || row_begin < 0 || n_rows < 0 || !out_counts) return MIDAS_SNPS_ERR_INVALID_ARG;
  const int64_t row_end = row_begin + n_rows;
  struct Task { size_t table, member; };
  std::vector<Task> tasks;
  for (size_t t = 0; t < ts->files.size(); ++t) {
    if (!out_counts[t]) continue;                // a table the caller reads some other way
    if (ts->rows[t] < row_end) {
      set_err(err256, "%s: rows up to %lld asked of a table that holds fewer (or does not say)", ts->paths[t].c_str(), (long long)row_end);
      return MIDAS_SNPS_ERR_INVALID_ARG;
    }
    for (size_t k = 0; k < ts->members[t].size(); ++k) {
      const TableSetMember& m = ts->members[t][k];
      if (m.row0 + m.rows > row_begin && m.row0 < row_end) tasks.push_back({t, k});
    }
  }
  std::atomic<long long> bad_row{-1};
  std::atomic<int> bad_table{-1}, corrupt{-1};
  run_pool(hw_threads(0), tasks.size(), [&](size_t i) {
    static thread_local std::vector<char> text;
    const Task& tk = tasks[i];
    const TableSetMember& m = ts->members[tk.table][tk.member];
    if (text.size() < m.ulen + 1) text.resize(m.ulen + 1);
    if (!raw_inflate(ts->files[tk.table].data() + m.data, (size_t)m.clen, reinterpret_cast<uint8_t*>(text.data()), (size_t)m.ulen)) { corrupt = (int)tk.table; return; }
    // rows of the member straight into the caller's array: the last four fields of every line (r[-4:],
    // midas/merge/snps.py:262-270), same checks as parse_rows
    const char* b = text.data();
    const char* const end = b + m.ulen;
    uint32_t* const dst = out_counts[tk.table];
    int64_t row = m.row0;
    while (b < end) {
      const char* nl = (const char*)memchr(b, '\n', (size_t)(end - b));
      const char* e = nl ? nl : end;
      if (row >= row_begin && row < row_end) {
        int n_tabs = 0;
        for (const char* q = b; q < e; ++q) n_tabs += *q == '\t';
        bool ok = n_tabs >= 7;
        uint32_t v4[4] = {0, 0, 0, 0};
        const char* q = e;
        for (int k = 3; k >= 0 && ok; --k) {      // backwards from the line's end: digits, then the tab in front of them
          uint64_t v = 0, scale = 1;
          const char* stop = q;
          while (q > b && q[-1] >= '0' && q[-1] <= '9') { v += (uint64_t)(q[-1] - '0') * scale; scale *= 10; --q; if (stop - q > 10) break; }
          if (q == stop || stop - q > 10 || v > 0x7FFFFFFFull || q == b || q[-1] != '\t') ok = false;
          v4[k] = (uint32_t)v;
          --q;
        }
        if (!ok) {
          long long none = -1;
          if (bad_row.compare_exchange_strong(none, (long long)row)) bad_table = (int)tk.table;
          return;
        }
        memcpy(dst + 4 * (row - row_begin), v4, 16);
      }
      ++row;
      b = nl ? nl + 1 : end;
    }
    if (row != m.row0 + m.rows) {               // the member holds another number of rows than it announces
      long long none = -1;
      if (bad_row.compare_exchange_strong(none, (long long)row)) bad_table = (int)tk.table;
    }
  });
  if (corrupt >= 0) { set_err(err256, "%s: corrupt deflate data", ts->paths[(size_t)corrupt.load()].c_str()); return MIDAS_SNPS_ERR_BAD_LAYOUT; }
  if (bad_row >= 0) {
    set_err(err256, "%s: malformed row %lld", ts->paths[(size_t)bad_table.load()].c_str(), bad_row.load() + 1);
    return MIDAS_SNPS_ERR_BAD_LAYOUT;
  }
  return MIDAS_SNPS_OK;
}

int32_t midas_snps_table_open(const char* path, int64_t max_rows, int32_t want_keys, midas_snps_table** out,
                              char* err256) {
  return midas_snps_table_open_range(path, 0, max_rows < 0 ? -1 : max_rows, want_keys, out, err256);
}

void midas_snps_table_close(midas_snps_table* t) { delete t; }
int64_t midas_snps_table_rows(const midas_snps_table* t) { return t ? t->rows : 0; }
int64_t midas_snps_table_key_bytes(const midas_snps_table* t) { return t ? t->key_bytes : 0; }
int32_t midas_snps_table_copy(const midas_snps_table* t, uint32_t* counts, char* keys, int64_t* key_off) {
  if (!t) return MIDAS_SNPS_ERR_INVALID_ARG;
  if (key_off) key_off[0] = 0;
  run_pool(hw_threads(0), t->pieces.size(), [&](size_t i) {   // every piece lands at its own offsets
    const int64_t take = t->take[i], skip = t->skip[i];
    if (take <= 0) return;
    const ParsedRows& pr = t->pieces[i];
    if (counts) memcpy(counts + 4 * t->row_base[i], pr.counts.data() + 4 * skip, (size_t)take * 16);
    if (!pr.key_end.empty()) {
      const int64_t k0 = skip > 0 ? pr.key_end[(size_t)skip - 1] : 0;     // key bytes in front of the wanted rows
      if (keys) memcpy(keys + t->key_base[i], pr.keys.data() + k0, (size_t)(pr.key_end[(size_t)(skip + take) - 1] - k0));
      if (key_off)
        for (int64_t r = 0; r < take; ++r) key_off[t->row_base[i] + r + 1] = t->key_base[i] + pr.key_end[(size_t)(skip + r)] - k0;
    }
  });
  return MIDAS_SNPS_OK;
}

namespace {
// Rows of any number of contigs -> gzip members of kRows rows, formatted and deflated by a pool, written in order.
int32_t write_contigs(const char* path, bool append, int32_t n_contigs, const char* const* ref_ids,
                      const int64_t* n_sites, const uint8_t* const* allele, const uint32_t* const* counts,
                      int32_t gz_level, int32_t threads, char* err256, bool header = true, const midas::RowFeed* feed = nullptr,
                      const int64_t* first_pos = nullptr) {
  // first_pos[k] (NULL: 0): entry k is a piece of its contig and its first row is position first_pos[k] + 1.  Members are cut
  // every kRowsPerMember rows from the entry's first row, so pieces that start at multiples of kRowsPerMember produce the
  // bytes the whole contig would.
  Lap lap("write rows");
  FILE* f = fopen(path, append ? "ab" : "wb");
  if (!f) { set_err(err256, "cannot open %s for writing", path); return MIDAS_SNPS_ERR_INVALID_ARG; }
  if (gz_level < 0 || gz_level > 9) gz_level = 6;
  bool ok = true;
  if (!append && header) {
    // header line of midas/run/snps.py:181-182
    static const char hdr[] = "ref_id\tref_pos\tref_allele\tdepth\tcount_a\tcount_c\tcount_g\tcount_t\n";
    std::vector<uint8_t> z;
    ok = gz_member(reinterpret_cast<const uint8_t*>(hdr), sizeof(hdr) - 1, gz_level, z) &&
         fwrite(z.data(), 1, z.size(), f) == z.size();
  }
  const int64_t kRows = midas::kRowsPerMember;   // rows per gzip member: enough members to keep every core busy on one species
  struct Chunk { int32_t contig; int64_t lo, hi; int32_t slab; int64_t in_slab; };
  std::vector<Chunk> chunks;
  std::vector<size_t> idlen((size_t)n_contigs);
  // With a feed the sites are not in host memory yet: they arrive slab by slab (a run of sites that is contiguous at the
  // source, whole members only) in a ring of the feed's slots, fetched by one thread while the others work on the
  // slab before.
  struct Slab { int64_t src_lo, n; int32_t chunks; const uint8_t* allele; const uint32_t* counts; };
  std::vector<Slab> slabs;
  for (int32_t k = 0; k < n_contigs; ++k) {
    idlen[(size_t)k] = strlen(ref_ids[k]);
    for (int64_t lo = 0; lo < n_sites[k]; lo += kRows) {
      const int64_t hi = std::min(n_sites[k], lo + kRows);
      Chunk ch{k, lo, hi, -1, 0};
      if (feed) {
        const int64_t src = feed->source_site[k] + lo;
        if (slabs.empty() || slabs.back().src_lo + slabs.back().n != src || slabs.back().n + (hi - lo) > feed->slab_sites)
          slabs.push_back({src, 0, 0, nullptr, nullptr});
        ch.slab = (int32_t)slabs.size() - 1;
        ch.in_slab = slabs.back().n;
        slabs.back().n += hi - lo;
        slabs.back().chunks += 1;
      }
      chunks.push_back(ch);
    }
  }
  const int64_t n_chunks = (int64_t)chunks.size();
  std::vector<std::atomic<int>> slab_ready(slabs.size()), slab_left(slabs.size());
  for (size_t k = 0; k < slabs.size(); ++k) { slab_ready[k] = 0; slab_left[k] = slabs[k].chunks; }
  int nt = writer_threads(threads);
  if ((int64_t)nt > n_chunks) nt = (int)std::max<int64_t>(1, n_chunks);
  std::vector<std::vector<uint8_t>> zbuf((size_t)n_chunks);
  std::vector<std::atomic<int>> done((size_t)n_chunks);
  for (auto& d : done) d = 0;
  std::atomic<int64_t> next{0};
  midas::Events events;      // chunk done / slab ready / slot free: the waits below sleep on it
  std::atomic<int> bad{0};
  // levels 1-5: the row coder (row_deflate.h: one table lookup per row, about zlib level 4's size at a fraction of its
  // time); 6-9: zlib at that level; 0: zlib, stored
  const bool row_coder = gz_level >= 1 && gz_level <= 5;
  auto work = [&] {
    std::vector<char> text;
    std::vector<uint32_t> row_at, tail_at;
    for (;;) {
      const int64_t ci = next.fetch_add(1);
      if (ci >= n_chunks) return;
      const Chunk& ch = chunks[(size_t)ci];
      const char* id = ref_ids[ch.contig];
      const size_t il = idlen[(size_t)ch.contig];
      const uint8_t* al;
      const uint32_t* cn;
      if (feed) {          // (pointers biased so that site i of the contig is al[i] / cn[4 i], as below)
        events.wait([&] { return slab_ready[(size_t)ch.slab].load(std::memory_order_acquire) != 0; });
        if (bad) return;
        al = slabs[(size_t)ch.slab].allele + ch.in_slab - ch.lo;
        cn = slabs[(size_t)ch.slab].counts + 4 * (ch.in_slab - ch.lo);
      } else {
        al = allele[ch.contig];
        cn = counts[ch.contig];
      }
      text.resize((size_t)(ch.hi - ch.lo) * (il + 80));
      row_at.resize((size_t)(ch.hi - ch.lo));
      tail_at.resize((size_t)(ch.hi - ch.lo));
      char* p = text.data();
      const int64_t row0 = first_pos ? first_pos[ch.contig] : 0;
      for (int64_t i = ch.lo; i < ch.hi; ++i) {
        // row = [contig.id, i+1, seq[i], depth, A, C, G, T] joined by tabs (midas/run/snps.py:202-210)
        row_at[(size_t)(i - ch.lo)] = (uint32_t)(p - text.data());
        memcpy(p, id, il); p += il;
        *p++ = '\t'; p = put_u64(p, (uint64_t)(row0 + i + 1));
        tail_at[(size_t)(i - ch.lo)] = (uint32_t)(p - text.data());
        *p++ = '\t'; *p++ = (char)al[i];
        const uint32_t* c = cn + 4 * i;
        *p++ = '\t'; p = put_u64(p, (uint64_t)c[0] + c[1] + c[2] + c[3]);
        *p++ = '\t'; p = put_u32(p, c[0]);
        *p++ = '\t'; p = put_u32(p, c[1]);
        *p++ = '\t'; p = put_u32(p, c[2]);
        *p++ = '\t'; p = put_u32(p, c[3]);
        *p++ = '\n';
      }
      const uint8_t* t8 = reinterpret_cast<const uint8_t*>(text.data());
      const size_t tn = (size_t)(p - text.data());
      const bool done_ok = row_coder ? gz_member_rows(t8, tn, row_at.data(), tail_at.data(), row_at.size(), zbuf[(size_t)ci], (uint32_t)(ch.hi - ch.lo))
                                     : gz_member(t8, tn, gz_level, zbuf[(size_t)ci], (uint32_t)(ch.hi - ch.lo));
      if (!done_ok) bad = 1;
      if (feed) slab_left[(size_t)ch.slab].fetch_sub(1, std::memory_order_release);
      done[(size_t)ci] = 1;
      events.signal();
    }
  };
  // (with a feed) one thread brings the slabs in, a ring slot being reused once every chunk of its previous slab is done
#ifdef MIDAS_HOSTIO_TRACE
  const auto t_begin = std::chrono::steady_clock::now();
#endif
  auto fetch = [&] {
    for (size_t k = 0; k < slabs.size(); ++k) {
      if (k >= (size_t)feed->n_slots)
        events.wait([&] { return slab_left[k - (size_t)feed->n_slots].load(std::memory_order_acquire) <= 0 || bad; });
#ifdef MIDAS_HOSTIO_TRACE
      const auto t0 = std::chrono::steady_clock::now();
#endif
      if (!bad && !feed->fetch(feed->user, (int)(k % (size_t)feed->n_slots), slabs[k].src_lo, slabs[k].n, &slabs[k].allele, &slabs[k].counts)) bad = 1;
#ifdef MIDAS_HOSTIO_TRACE
      fprintf(stderr, "[write rows] slab %zu of %zu: %lld sites, %d members, fetched in %.2f ms (waited for the slot until %.2f ms)\n", k, slabs.size(),
              (long long)slabs[k].n, slabs[k].chunks, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(),
              std::chrono::duration<double, std::milli>(t0 - t_begin).count());
#endif
      if (bad) {          // let everybody out
        for (size_t j = k; j < slabs.size(); ++j) slab_ready[j].store(1, std::memory_order_release);
        for (auto& d : done) d = 1;
        events.signal();
        return;
      }
      slab_ready[k].store(1, std::memory_order_release);
      events.signal();
    }
  };
  // one thread writes the finished chunks in order while the others format / compress the next ones
  auto drain = [&] {
    for (int64_t ci = 0; ci < n_chunks && ok; ++ci) {
      events.wait([&] { return done[(size_t)ci].load() != 0; });
      if (bad) { ok = false; break; }
      std::vector<uint8_t>& z = zbuf[(size_t)ci];
      ok = fwrite(z.data(), 1, z.size(), f) == z.size();
      std::vector<uint8_t>().swap(z);
    }
    if (!ok) { next = n_chunks; bad = 1; events.signal(); }   // stop the pool (and the slab feeder)
  };
  std::atomic<int> role{0};
  lap("setup");
  // roles: with a feed the calling thread brings the slabs in (it is the one thread that has already talked to the
  // device -- a pool thread's first HIP call costs ~13 ms of per-thread set-up) and joins the formatters afterwards; the
  // first of the others writes, the rest format
  const bool feeding = feed && !slabs.empty();
  const std::thread::id caller = std::this_thread::get_id();
  Workers::run(nt + (feeding ? 2 : 1), [&] {
    if (feeding && std::this_thread::get_id() == caller) {
      fetch();
      work();
      if (role.fetch_add(1) == 0) drain();     // (no other thread has arrived yet: a tiny table on a slow-to-wake pool)
      return;
    }
    if (role.fetch_add(1) == 0) drain(); else work();
  });
  lap("format + gzip + write");
  if (fclose(f) != 0) ok = false;
  lap("fclose");
  if (!ok || bad) { set_err(err256, "write failed on %s", path); return MIDAS_SNPS_ERR_INVALID_ARG; }
  return MIDAS_SNPS_OK;
}
}  // namespace

}  // extern "C"
namespace midas {
int32_t write_coded_members(const char* path, bool with_header, int32_t gz_level, int64_t n_members, const CodedMember* members,
                            int32_t threads, char* err256) {
  Lap lap("write coded members");
  std::vector<uint8_t> head;
  if (with_header) {
    static const char hdr[] = "ref_id\tref_pos\tref_allele\tdepth\tcount_a\tcount_c\tcount_g\tcount_t\n";
    if (gz_level < 0 || gz_level > 9) gz_level = 6;
    if (!gz_member(reinterpret_cast<const uint8_t*>(hdr), sizeof(hdr) - 1, gz_level, head)) {
      set_err(err256, "cannot compress the header line of %s", path);
      return MIDAS_SNPS_ERR_INVALID_ARG;
    }
  }
  std::vector<uint64_t> at((size_t)n_members + 1);
  at[0] = head.size();
  for (int64_t k = 0; k < n_members; ++k) at[(size_t)k + 1] = at[(size_t)k] + kGzHeader + members[k].n_bytes + 8u;
  const int fd = open(path, O_WRONLY | O_CREAT | O_TRUNC, 0666);
  if (fd < 0) { set_err(err256, "cannot open %s for writing", path); return MIDAS_SNPS_ERR_INVALID_ARG; }
  std::atomic<int> bad{0};
  auto write_all = [&](struct iovec* v, int n_iov, uint64_t off) {     // (consumes v)
    int first = 0;
    while (first < n_iov) {
      const ssize_t got = pwritev(fd, v + first, std::min(n_iov - first, 1024), (off_t)off);
      if (got <= 0) { bad = 1; return; }
      off += (uint64_t)got;
      size_t left = (size_t)got;
      while (first < n_iov && left >= v[first].iov_len) { left -= v[first].iov_len; ++first; }
      if (first < n_iov) { v[first].iov_base = static_cast<uint8_t*>(v[first].iov_base) + left; v[first].iov_len -= left; }
    }
  };
  if (!head.empty()) { struct iovec v{head.data(), head.size()}; write_all(&v, 1, 0); }
  // One file takes buffered writes from one thread at a time (the inode's lock), at 2-3 GB/s: the members go out from the
  // calling thread, hundreds per pwritev.  Callers with several tables to write (one per species) write them side by side.
  (void)threads;
  constexpr int64_t kBatch = 256;          // 3 iovecs a member, IOV_MAX is 1024
  std::vector<uint8_t> frames((size_t)kBatch * (kGzHeader + 8));
  std::vector<struct iovec> iov((size_t)kBatch * 3);
  for (int64_t k0 = 0; k0 < n_members && !bad; k0 += kBatch) {
    const int64_t k1 = std::min(n_members, k0 + kBatch);
    for (int64_t k = k0; k < k1; ++k) {
      const CodedMember& m = members[k];
      const uint64_t total = kGzHeader + (uint64_t)m.n_bytes + 8u;
      uint8_t* frame = frames.data() + (size_t)(k - k0) * (kGzHeader + 8);
      const uint8_t fixed[kGzHeader] = {0x1f, 0x8b, 8, 4 /* FEXTRA */, 0, 0, 0, 0, 0, 255, 16, 0, 'M', 'S', 4, 0,
                                        (uint8_t)total, (uint8_t)(total >> 8), (uint8_t)(total >> 16), (uint8_t)(total >> 24),
                                        'M', 'R', 4, 0, (uint8_t)m.rows, (uint8_t)(m.rows >> 8), (uint8_t)(m.rows >> 16), (uint8_t)(m.rows >> 24)};
      memcpy(frame, fixed, kGzHeader);
      memcpy(frame + kGzHeader, &m.crc, 4);
      memcpy(frame + kGzHeader + 4, &m.text_len, 4);
      iov[(size_t)(k - k0) * 3] = {frame, kGzHeader};
      iov[(size_t)(k - k0) * 3 + 1] = {const_cast<uint8_t*>(m.data), m.n_bytes};
      iov[(size_t)(k - k0) * 3 + 2] = {frame + kGzHeader, 8};
    }
    write_all(iov.data(), (int)(k1 - k0) * 3, at[(size_t)k0]);
  }
  lap("frame + write");
  if (close(fd) != 0) bad = 1;
  if (bad) { set_err(err256, "write failed on %s", path); return MIDAS_SNPS_ERR_INVALID_ARG; }
  return MIDAS_SNPS_OK;
}

int32_t write_rows_fed(const char* path, bool with_header, int32_t n_contigs, const char* const* ref_ids, const int64_t* n_sites,
                       int32_t gz_level, int32_t threads, const RowFeed& feed, char* err256, const int64_t* first_pos) {
  return write_contigs(path, false, n_contigs, ref_ids, n_sites, nullptr, nullptr, gz_level, threads, err256, with_header, &feed, first_pos);
}
}  // namespace midas
extern "C" {

int32_t midas_snps_deflate_rows(const uint8_t* text, int64_t n, const uint32_t* row_begin, const uint32_t* tail_begin,
                                int64_t n_rows, uint8_t* out, int64_t out_cap, int64_t* out_len) {
  if (!text || n <= 0 || n > 0x7FFFFFFFll || n_rows < 0 || (n_rows > 0 && (!row_begin || !tail_begin)) || !out || !out_len)
    return MIDAS_SNPS_ERR_INVALID_ARG;
  for (int64_t k = 0; k < n_rows; ++k) {
    const int64_t end = k + 1 < n_rows ? (int64_t)row_begin[k + 1] : n;
    if ((k == 0 ? 0 : (int64_t)row_begin[k - 1]) > (int64_t)row_begin[k] || row_begin[k] > tail_begin[k] || (int64_t)tail_begin[k] >= end)
      return MIDAS_SNPS_ERR_INVALID_ARG;
  }
  std::vector<uint8_t> z;
  midas::RowDeflate coder;
  coder.compress(text, (size_t)n, row_begin, tail_begin, (size_t)n_rows, z);
  if ((int64_t)z.size() > out_cap) return MIDAS_SNPS_ERR_INVALID_ARG;
  memcpy(out, z.data(), z.size());
  *out_len = (int64_t)z.size();
  return MIDAS_SNPS_OK;
}

int32_t midas_snps_write_rows(const char* path, int32_t append, const char* ref_id, int64_t n_sites,
                              const uint8_t* allele, const uint32_t* counts, int32_t gz_level, int32_t threads,
                              char* err256) {
  if (!path || (n_sites > 0 && (!ref_id || !allele || !counts)) || n_sites < 0) return MIDAS_SNPS_ERR_INVALID_ARG;
  const char* id = ref_id ? ref_id : "";
  return write_contigs(path, append != 0, n_sites > 0 ? 1 : 0, &id, &n_sites, &allele, &counts, gz_level, threads, err256);
}

int32_t midas_snps_write_table(const char* path, int32_t n_contigs, const char* const* ref_ids, const int64_t* n_sites,
                               const uint8_t* const* allele, const uint32_t* const* counts, int32_t gz_level,
                               int32_t threads, char* err256) {
  if (!path || n_contigs < 0 || (n_contigs > 0 && (!ref_ids || !n_sites || !allele || !counts)))
    return MIDAS_SNPS_ERR_INVALID_ARG;
  for (int32_t k = 0; k < n_contigs; ++k)
    if (!ref_ids[k] || n_sites[k] < 0 || (n_sites[k] > 0 && (!allele[k] || !counts[k]))) return MIDAS_SNPS_ERR_INVALID_ARG;
  return write_contigs(path, false, n_contigs, ref_ids, n_sites, allele, counts, gz_level, threads, err256);
}

int32_t midas_snps_write_part(const char* path, int32_t with_header, int32_t n_contigs, const char* const* ref_ids,
                              const int64_t* n_sites, const uint8_t* const* allele, const uint32_t* const* counts,
                              int32_t gz_level, int32_t threads, char* err256) {
  if (!path || n_contigs < 0 || (n_contigs > 0 && (!ref_ids || !n_sites || !allele || !counts)))
    return MIDAS_SNPS_ERR_INVALID_ARG;
  for (int32_t k = 0; k < n_contigs; ++k)
    if (!ref_ids[k] || n_sites[k] < 0 || (n_sites[k] > 0 && (!allele[k] || !counts[k]))) return MIDAS_SNPS_ERR_INVALID_ARG;
  return write_contigs(path, false, n_contigs, ref_ids, n_sites, allele, counts, gz_level, threads, err256, with_header != 0);
}

int32_t midas_snps_write_pieces(const char* path, int32_t with_header, int32_t n_contigs, const char* const* ref_ids,
                                const int64_t* n_sites, const int64_t* first_pos, const uint8_t* const* allele,
                                const uint32_t* const* counts, int32_t gz_level, int32_t threads, char* err256) {
  if (!path || n_contigs < 0 || (n_contigs > 0 && (!ref_ids || !n_sites || !allele || !counts)))
    return MIDAS_SNPS_ERR_INVALID_ARG;
  for (int32_t k = 0; k < n_contigs; ++k)
    if (!ref_ids[k] || n_sites[k] < 0 || (n_sites[k] > 0 && (!allele[k] || !counts[k])) || (first_pos && first_pos[k] < 0))
      return MIDAS_SNPS_ERR_INVALID_ARG;
  return write_contigs(path, false, n_contigs, ref_ids, n_sites, allele, counts, gz_level, threads, err256, with_header != 0, nullptr, first_pos);
}

int32_t midas_merge_write_matrix(const char* path, const char* header_line, int64_t n_keep, const int64_t* keep,
                                 int32_t n_samples, int64_t n_sites, const uint32_t* depth, const uint32_t* minor_count,
                                 int32_t threads, int64_t site_id_base, char* err256) {
  if (!path || !header_line || n_keep < 0 || n_samples <= 0 || n_sites < 0 || (n_keep > 0 && (!keep || !depth)))
    return MIDAS_SNPS_ERR_INVALID_ARG;
  FILE* f = fopen(path, "wb");
  if (!f) { set_err(err256, "cannot open %s for writing", path); return MIDAS_SNPS_ERR_INVALID_ARG; }
  bool ok = fwrite(header_line, 1, strlen(header_line), f) == strlen(header_line);
  const int64_t kRows = 1 << 13;
  const int64_t n_chunks = (n_keep + kRows - 1) / kRows;
  int nt = writer_threads(threads);
  if ((int64_t)nt > n_chunks) nt = (int)std::max<int64_t>(1, n_chunks);
  std::vector<std::vector<char>> text((size_t)n_chunks);
  std::vector<std::atomic<int>> done((size_t)n_chunks);
  for (auto& d : done) d = 0;
  std::atomic<int64_t> next{0};
  midas::Events events;      // chunk done / slab ready / slot free: the waits below sleep on it
  auto work = [&] {
    for (;;) {
      const int64_t ci = next.fetch_add(1);
      if (ci >= n_chunks) return;
      const int64_t lo = ci * kRows, hi = std::min(n_keep, lo + kRows);
      std::vector<char>& t = text[(size_t)ci];
      t.resize((size_t)(hi - lo) * (24 + 16 * (size_t)n_samples));
      char* p = t.data();
      for (int64_t r = lo; r < hi; ++r) {
        const int64_t i = keep[r];
        p = put_u64(p, (uint64_t)(site_id_base + i + 1));                    // site_id = 1-based table row
        for (int32_t s = 0; s < n_samples; ++s) {
          *p++ = '\t';
          const uint32_t d = depth[(size_t)s * (size_t)n_sites + (size_t)i];
          if (!minor_count) {
            p = put_u32(p, d);                                               // str(depth)
          } else {
            // '{0:.3g}'.format(float(minor) / depth if depth > 0 else 0.0)  (midas/merge/snps.py:88-90, 197)
            const uint32_t m = minor_count[(size_t)s * (size_t)n_sites + (size_t)i];
            if (d == 0 || m == 0) *p++ = '0';
            else p += snprintf(p, 16, "%.3g", (double)m / (double)d);
          }
        }
        *p++ = '\n';
      }
      t.resize((size_t)(p - t.data()));
      done[(size_t)ci] = 1;
      events.signal();
    }
  };
  // one thread writes the finished chunks in order while the others format / compress the next ones
  auto drain = [&] {
    for (int64_t ci = 0; ci < n_chunks && ok; ++ci) {
      events.wait([&] { return done[(size_t)ci].load() != 0; });
      std::vector<char>& t = text[(size_t)ci];
      ok = fwrite(t.data(), 1, t.size(), f) == t.size();
      std::vector<char>().swap(t);
    }
    if (!ok) next = n_chunks;
  };
  std::atomic<int> role{0};
  Workers::run(nt + 1, [&] { if (role.fetch_add(1) == 0) drain(); else work(); });
  if (fclose(f) != 0) ok = false;
  if (!ok) { set_err(err256, "write failed on %s", path); return MIDAS_SNPS_ERR_INVALID_ARG; }
  return MIDAS_SNPS_OK;
}

namespace {
// the standard genetic code in the reference's spelling (stop = '_'), indexed by 16*b0 + 4*b1 + b2 with T,C,A,G = 0..3
const char kAmino[65] = "FFLLSSSSYY__CC_WLLLLPPPPHHQQRRRRIIIMTTTTNNKKSSRRVVVVAAAADDEEGGGG";
inline int base_index(char b) { return b == 'T' ? 0 : b == 'C' ? 1 : b == 'A' ? 2 : b == 'G' ? 3 : -1; }
inline char complement_base(char b) { return b == 'A' ? 'T' : b == 'T' ? 'A' : b == 'G' ? 'C' : b == 'C' ? 'G' : b; }
}  // namespace

int32_t midas_merge_write_info(const char* path, const char* header_line, int64_t n_keep, const int64_t* keep,
                               const char* keys, const int64_t* key_off, const uint8_t* calls,
                               const uint32_t* count_samples, const uint64_t* pooled, const midas_merge_genes* genes,
                               int32_t threads, int64_t site_id_base, char* err256) {
  if (!path || !header_line || n_keep < 0 || !genes || genes->n_genes < 0 ||
      (n_keep > 0 && (!keep || !keys || !key_off || !calls || !count_samples || !pooled)) ||
      (genes->n_genes > 0 && (!genes->scaffold_id || !genes->start || !genes->end || !genes->strand || !genes->gene_type ||
                              !genes->gene_id || !genes->seq)))
    return MIDAS_SNPS_ERR_INVALID_ARG;
  FILE* f = fopen(path, "wb");
  if (!f) { set_err(err256, "cannot open %s for writing", path); return MIDAS_SNPS_ERR_INVALID_ARG; }
  bool ok = fwrite(header_line, 1, strlen(header_line), f) == strlen(header_line);
  const int64_t ng = genes->n_genes;
  std::vector<size_t> seq_len((size_t)ng), sid_len((size_t)ng);
  std::vector<char> is_cds((size_t)ng);
  for (int64_t g = 0; g < ng; ++g) {
    seq_len[(size_t)g] = strlen(genes->seq[g]);
    sid_len[(size_t)g] = strlen(genes->scaffold_id[g]);
    is_cds[(size_t)g] = strcmp(genes->gene_type[g], "CDS") == 0;
  }
  // Python's str comparison (code points) is byte order for the ASCII ids of a MIDAS database
  auto cmp_id = [&](const char* a, size_t la, int64_t g) {
    const size_t lb = sid_len[(size_t)g];
    const int c = memcmp(a, genes->scaffold_id[g], la < lb ? la : lb);
    return c != 0 ? c : (la < lb ? -1 : (la > lb ? 1 : 0));
  };
  const int64_t kRows = 1 << 13;
  const int64_t n_chunks = (n_keep + kRows - 1) / kRows;
  int nt = writer_threads(threads);
  if ((int64_t)nt > n_chunks) nt = (int)std::max<int64_t>(1, n_chunks);
  std::vector<std::string> text((size_t)n_chunks);
  std::vector<std::atomic<int>> done((size_t)n_chunks);
  for (auto& d : done) d = 0;
  std::atomic<int64_t> next{0};
  midas::Events events;      // chunk done / slab ready / slot free: the waits below sleep on it
  static const char* kSnpType[5] = {"NA", "mono", "bi", "tri", "quad"};
  auto work = [&] {
    char num[24];
    for (;;) {
      const int64_t ci = next.fetch_add(1);
      if (ci >= n_chunks) return;
      const int64_t lo = ci * kRows, hi = std::min(n_keep, lo + kRows);
      std::string& t = text[(size_t)ci];
      t.reserve((size_t)(hi - lo) * 96);
      int64_t cursor = 0;   // the reference's forward cursor: a gene behind a site is behind every later site, so the
                            // cursor before a site is simply the first gene not behind it -- chunks can start from 0
      for (int64_t r = lo; r < hi; ++r) {
        const int64_t i = keep[r];
        const char* key = keys + key_off[i];
        const size_t klen = (size_t)(key_off[i + 1] - key_off[i]);
        // rsplit('|', 2)
        size_t p2 = klen;
        while (p2 > 0 && key[p2 - 1] != '|') --p2;
        size_t p1 = p2 > 0 ? p2 - 1 : 0;
        while (p1 > 0 && key[p1 - 1] != '|') --p1;
        if (p2 == 0 || p1 == 0) { t.append("malformed key\n"); continue; }
        const char* ref_id = key;
        const size_t id_len = p1 - 1;
        long long ref_pos = 0;
        for (size_t q = p1; q + 1 < p2; ++q) ref_pos = ref_pos * 10 + (key[q] - '0');
        // ---- annotate -----------------------------------------------------------------------------------
        const char* locus = "IGR";
        const char* gene_id = "NA";
        char site_type[4] = "NA";
        char aas[8] = "NA";
        while (cursor < ng) {
          const int c = cmp_id(ref_id, id_len, cursor);
          if (c < 0 || (c == 0 && ref_pos < genes->start[cursor])) break;             // upstream of the next gene
          if (c > 0 || (c == 0 && ref_pos > genes->end[cursor])) { ++cursor; continue; }   // gene is behind the site
          locus = genes->gene_type[cursor];
          gene_id = genes->gene_id[cursor];
          if (is_cds[(size_t)cursor] && seq_len[(size_t)cursor] % 3 == 0) {
            const bool plus = genes->strand[cursor] == '+';
            const long long gpos = plus ? ref_pos - genes->start[cursor] : genes->end[cursor] - ref_pos;
            const long long cpos = gpos % 3;
            const long long c0 = gpos - cpos;
            const char* sq = genes->seq[cursor];
            if (c0 >= 0 && (size_t)(c0 + 3) <= seq_len[(size_t)cursor]) {
              int b[3] = {base_index(sq[c0]), base_index(sq[c0 + 1]), base_index(sq[c0 + 2])};
              if (b[0] >= 0 && b[1] >= 0 && b[2] >= 0) {
                char aa[4];
                int distinct = 0;
                for (int a = 0; a < 4; ++a) {
                  const char allele = "ACGT"[a];
                  int bb[3] = {b[0], b[1], b[2]};
                  bb[cpos] = base_index(plus ? allele : complement_base(allele));
                  aa[a] = kAmino[16 * bb[0] + 4 * bb[1] + bb[2]];
                  bool seen = false;
                  for (int x = 0; x < a; ++x) seen |= aa[x] == aa[a];
                  distinct += !seen;
                }
                snprintf(site_type, sizeof site_type, "%dD", 5 - distinct);
                snprintf(aas, sizeof aas, "%c,%c,%c,%c", aa[0], aa[1], aa[2], aa[3]);
              }
            }
          }
          break;
        }
        // ---- the line -----------------------------------------------------------------------------------
        const uint8_t* cl = calls + 4 * i;
        auto put = [&](uint64_t v) { char* e = put_u64(num, v); t.append(num, (size_t)(e - num)); };
        put((uint64_t)(site_id_base + i + 1)); t.push_back('\t');
        t.append(ref_id, id_len); t.push_back('\t');
        put((uint64_t)ref_pos); t.push_back('\t');
        t.append(key + p2, klen - p2); t.push_back('\t');
        if (cl[0] < 4) t.push_back("ACGT"[cl[0]]); else t.append("NA");
        t.push_back('\t');
        if (cl[1] < 4) t.push_back("ACGT"[cl[1]]); else t.append("NA");
        t.push_back('\t');
        put(count_samples[i]); t.push_back('\t');
        for (int a = 0; a < 4; ++a) { put(pooled[4 * i + a]); t.push_back('\t'); }
        t.append(locus); t.push_back('\t');
        t.append(gene_id); t.push_back('\t');
        t.append(kSnpType[cl[2] < 5 ? cl[2] : 0]); t.push_back('\t');
        t.append(site_type); t.push_back('\t');
        t.append(aas); t.push_back('\n');
      }
      done[(size_t)ci] = 1;
      events.signal();
    }
  };
  // one thread writes the finished chunks in order while the others format / compress the next ones
  auto drain = [&] {
    for (int64_t ci = 0; ci < n_chunks && ok; ++ci) {
      events.wait([&] { return done[(size_t)ci].load() != 0; });
      std::string& t = text[(size_t)ci];
      ok = fwrite(t.data(), 1, t.size(), f) == t.size();
      std::string().swap(t);
    }
    if (!ok) next = n_chunks;
  };
  std::atomic<int> role{0};
  Workers::run(nt + 1, [&] { if (role.fetch_add(1) == 0) drain(); else work(); });
  if (fclose(f) != 0) ok = false;
  if (!ok) { set_err(err256, "write failed on %s", path); return MIDAS_SNPS_ERR_INVALID_ARG; }
  return MIDAS_SNPS_OK;
}

}  // extern "C"
