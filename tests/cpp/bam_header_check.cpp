// The pure pieces of the host's BAM reader (midas_amd/csrc/bam_parse.h) held to what they promise: the header parser on every
// prefix of a header (each in a heap buffer of exactly its size, so that a read behind it is seen) and on broken ones, and the
// two searches over a block table against a linear scan.
// Stand-alone: prints "ok <checks>" and returns 0, or says what failed and returns 1.
#include "bam_parse.h"

#include <cstdio>
#include <cstdlib>

using namespace midas;

static long long n_checks = 0;
#define CHECK(cond, ...)                                       \
  do {                                                         \
    ++n_checks;                                                \
    if (!(cond)) {                                             \
      printf("FAILED %s:%d: %s: ", __FILE__, __LINE__, #cond); \
      printf(__VA_ARGS__);                                     \
      printf("\n");                                            \
      exit(1);                                                 \
    }                                                          \
  } while (0)

static void put32(std::vector<uint8_t>& v, uint32_t x) { for (int k = 0; k < 4; ++k) v.push_back((uint8_t)(x >> (8 * k))); }
static std::vector<uint8_t> make_header(const std::string& text, const std::vector<std::string>& names, const std::vector<int64_t>& lens) {
  std::vector<uint8_t> v = {'B', 'A', 'M', 1};
  put32(v, (uint32_t)text.size());
  v.insert(v.end(), text.begin(), text.end());
  put32(v, (uint32_t)names.size());
  for (size_t i = 0; i < names.size(); ++i) {
    put32(v, (uint32_t)names[i].size() + 1);
    v.insert(v.end(), names[i].begin(), names[i].end());
    v.push_back(0);
    put32(v, (uint32_t)lens[i]);
  }
  return v;
}
// the parser on the first n bytes of `bytes`, copied into a heap buffer of exactly n
static BamHeader parse_prefix(const std::vector<uint8_t>& bytes, size_t n, std::vector<std::string>* names, std::vector<int64_t>* lens, size_t* rec_begin) {
  uint8_t* d = static_cast<uint8_t*>(malloc(n ? n : 1));
  if (n) memcpy(d, bytes.data(), n);
  const BamHeader r = parse_bam_header(n ? d : nullptr, n, names, lens, rec_begin);
  free(d);
  return r;
}

static void check_headers() {
  const std::vector<std::string> all_names = {"contig_1", "c", "a_much_longer_reference_name"};
  const std::vector<int64_t> all_lens = {1000, 1, 2000000000};
  for (size_t n_ref : {0, 1, 3}) {
    const std::vector<std::string> want_names(all_names.begin(), all_names.begin() + n_ref);
    const std::vector<int64_t> want_lens(all_lens.begin(), all_lens.begin() + n_ref);
    std::vector<uint8_t> h = make_header("@HD\tVN:1.0\tSO:coordinate\n", want_names, want_lens);
    const size_t full = h.size();
    for (int k = 0; k < 100; ++k) h.push_back((uint8_t)(37 * k + 1));      // (what follows the header: records, here noise)
    std::vector<std::string> names;
    std::vector<int64_t> lens;
    size_t rec_begin = 0;
    for (size_t n = 0; n < full; ++n)
      CHECK(parse_prefix(h, n, &names, &lens, &rec_begin) == BamHeader::more, "%zu references, prefix of %zu bytes of %zu", n_ref, n, full);
    for (size_t n : {full, full + 100}) {
      rec_begin = 0;
      CHECK(parse_prefix(h, n, &names, &lens, &rec_begin) == BamHeader::parsed, "%zu references, all %zu bytes", n_ref, n);
      CHECK(names == want_names && lens == want_lens && rec_begin == full, "%zu references: %zu names, %zu lengths, rec_begin %zu of %zu", n_ref,
            names.size(), lens.size(), rec_begin, full);
    }
  }
  std::vector<std::string> names;
  std::vector<int64_t> lens;
  size_t rec_begin = 0;
  // the first four bytes are wrong
  std::vector<uint8_t> h = make_header("@HD\n", all_names, all_lens);
  h[3] = 2;
  CHECK(parse_prefix(h, h.size(), &names, &lens, &rec_begin) == BamHeader::bad_magic, "magic BAM\\2");
  // l_name == 0 in the second reference
  h = make_header("@HD\n", all_names, all_lens);
  const size_t second = 4 + 4 + 4 + 4 + (4 + all_names[0].size() + 1 + 4);
  CHECK(h[second] == all_names[1].size() + 1, "the second reference's l_name is at %zu", second);
  h[second] = 0;
  CHECK(parse_prefix(h, h.size(), &names, &lens, &rec_begin) == BamHeader::bad_refs, "l_name == 0");
  CHECK(parse_prefix(h, second + 4, &names, &lens, &rec_begin) == BamHeader::bad_refs, "l_name == 0 at the buffer's end");
  CHECK(parse_prefix(h, second + 3, &names, &lens, &rec_begin) == BamHeader::more, "l_name == 0 not yet in the buffer");
  // l_text points past the buffer: by a little, and by all a u32 can say
  for (uint32_t l_text : {5u, 1000000u, 0xFFFFFFFFu}) {
    h = make_header("@HD\n", all_names, all_lens);
    h.resize(4 + 4 + 4 + 4);
    memcpy(&h[4], &l_text, 4);
    CHECK(parse_prefix(h, h.size(), &names, &lens, &rec_begin) == BamHeader::more, "l_text %u in %zu bytes", l_text, h.size());
  }
}

struct Blk { uint64_t upos; uint32_t ulen; size_t fpos; };
static void check_searches() {
  // irregular sizes; the 17-block table has empty blocks inside and the empty EOF block at its end
  const uint32_t ulens[17] = {65280, 1, 300, 0, 65280, 7, 7, 1, 0, 0, 12345, 2, 65279, 1, 9, 64, 0};
  const uint32_t clens[17] = {20000, 40, 99, 28, 65000, 35, 36, 29, 28, 28, 5000, 31, 777, 30, 41, 50, 28};
  for (size_t nb : {0, 1, 2, 17}) {
    std::vector<Blk> t;
    uint64_t total = 0;
    size_t size = 0;
    for (size_t i = 0; i < nb; ++i) {
      t.push_back({total, ulens[i], size});
      total += ulens[i];
      size += clens[i];
    }
    for (uint64_t u = 0; u <= total; ++u) {
      size_t want = 0;
      while (want < nb && t[want].upos + t[want].ulen <= u) ++want;
      const size_t got = block_holding(t.data(), nb, u);
      CHECK(got == want, "%zu blocks, u = %llu: block %zu, a scan says %zu", nb, (unsigned long long)u, got, want);
      if (u < total) CHECK(t[got].upos <= u && u < t[got].upos + t[got].ulen, "%zu blocks: block %zu does not hold %llu", nb, got, (unsigned long long)u);
    }
    for (size_t f = 0; f <= size; ++f) {
      size_t want = 0;
      while (want < nb && t[want].fpos < f) ++want;
      const size_t got = first_block_at(t.data(), nb, f);
      CHECK(got == want, "%zu blocks, fpos = %zu: block %zu, a scan says %zu", nb, f, got, want);
    }
  }
}

int main() {
  check_headers();
  check_searches();
  printf("ok %lld\n", n_checks);
  return 0;
}
