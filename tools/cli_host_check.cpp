// cli_host_check.cpp -- the host pieces of the `scalce` tool (scalce_amd/csrc/cli_io.hpp, cli_input.hpp, cli_shares.hpp,
// cli_sink.hpp, cli_sidefiles.hpp) on their own: a program for AddressSanitizer and UBSan, no device, no HIP.
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/cli_host_check.cpp -lz -lpthread -o /tmp/chk && /tmp/chk
// It works on small files it writes itself, in the directory given as its argument (or one it makes under /tmp), and
// prints "cli_host_check: ok".
#include <dirent.h>

#include "../scalce_amd/csrc/cli_input.hpp"
#include "../scalce_amd/csrc/cli_io.hpp"
#include "../scalce_amd/csrc/cli_shares.hpp"
#include "../scalce_amd/csrc/cli_sidefiles.hpp"
#include "../scalce_amd/csrc/cli_sink.hpp"

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #x); exit(1); } } while (0)

typedef std::vector<uint8_t> Bytes;
static std::string g_dir;
static std::string in_dir(const std::string &name) { return g_dir + "/" + name; }

static std::string put(const std::string &name, const void *p, size_t n) {
  const std::string path = in_dir(name);
  FILE *f = fopen(path.c_str(), "wb");
  CHECK(f && fwrite(p, 1, n, f) == n);
  fclose(f);
  return path;
}
static std::string put(const std::string &name, const std::string &s) { return put(name, s.data(), s.size()); }
static Bytes get(const std::string &path) {
  FILE *f = fopen(path.c_str(), "rb");
  CHECK(f);
  Bytes out;
  uint8_t buf[65536];
  for (size_t k; (k = fread(buf, 1, sizeof buf, f)) > 0;) out.insert(out.end(), buf, buf + k);
  fclose(f);
  return out;
}
static Bytes bytes_of(const std::string &s) { return Bytes(s.begin(), s.end()); }
static int open_descriptors() {
  DIR *d = opendir("/proc/self/fd");
  CHECK(d);
  int n = 0;
  while (readdir(d)) n++;
  closedir(d);
  return n;
}
static std::string gzip_of(const std::string &s) {  // one member
  z_stream z;
  memset(&z, 0, sizeof z);
  CHECK(deflateInit2(&z, 6, Z_DEFLATED, 15 + 16, 8, Z_DEFAULT_STRATEGY) == Z_OK);
  std::string out(deflateBound(&z, (uLong)s.size()) + 64, '\0');
  z.next_in = reinterpret_cast<Bytef *>(const_cast<char *>(s.data())); z.avail_in = (uInt)s.size();
  z.next_out = reinterpret_cast<Bytef *>(&out[0]); z.avail_out = (uInt)out.size();
  CHECK(deflate(&z, Z_FINISH) == Z_STREAM_END);
  out.resize(z.total_out);
  deflateEnd(&z);
  return out;
}
static Bytes gunzip_members(const Bytes &gzb) {  // concatenated members, each complete
  Bytes out, buf(1u << 20);
  z_stream z;
  memset(&z, 0, sizeof z);
  CHECK(inflateInit2(&z, 15 + 16) == Z_OK);
  z.next_in = const_cast<Bytef *>(gzb.data()); z.avail_in = (uInt)gzb.size();
  CHECK(z.avail_in > 0);
  for (;;) {
    z.next_out = buf.data(); z.avail_out = (uInt)buf.size();
    const int rc = inflate(&z, Z_NO_FLUSH);
    CHECK(rc == Z_OK || rc == Z_STREAM_END);
    out.insert(out.end(), buf.begin(), buf.begin() + (buf.size() - z.avail_out));
    if (rc == Z_STREAM_END) {
      if (!z.avail_in) break;
      CHECK(inflateReset(&z) == Z_OK);
    }
  }
  inflateEnd(&z);
  return out;
}

// ---- FASTQ text: records whose names (and so whose lengths) differ, so that byte N-ths of a file fall inside lines -------
struct Fastq {
  std::string text;
  std::vector<uint64_t> rec;  // where record i starts; rec[n] = the size
};
static Fastq fastq(int n, int L, unsigned seed, bool equal_records = false) {
  Fastq f;
  for (int i = 0; i < n; i++) {
    f.rec.push_back(f.text.size());
    char name[64];
    snprintf(name, sizeof name, equal_records ? "@r%04d" : "@r%d", i);
    f.text += name;
    if (!equal_records) f.text.append((size_t)((i * 7 + seed) % 13), 'x');
    f.text += '\n';
    for (int j = 0; j < L; j++) f.text += "ACGT"[(i * 31 + j * 7 + seed) & 3];
    f.text += "\n+\n";
    for (int j = 0; j < L; j++) f.text += (char)(33 + (i * 5 + j * 3 + seed) % 40);
    f.text += '\n';
  }
  f.rec.push_back(f.text.size());
  return f;
}

// ---- record cuts: every rank's part of the exchange, computed in this one process -----------------------------------------
static std::vector<uint64_t> tentative(int fd, uint64_t size, int world) {  // what the all-gather would hand to every rank
  std::vector<uint64_t> g((size_t)world * 2);
  for (int r = 0; r < world; r++) {
    const uint64_t a = line_start(fd, size, world, r), b = line_start(fd, size, world, r + 1);
    CHECK(a <= b && b <= size);
    g[2 * r] = count_newlines(fd, a, b, 3);
    g[2 * r + 1] = a;
  }
  return g;
}
static void check_cuts_of(const Fastq &a, const Fastq &b, const char *what) {
  const int n = (int)a.rec.size() - 1;
  CHECK(b.rec.size() == a.rec.size());
  const std::string pa = put(std::string(what) + "_1.fq", a.text), pb = put(std::string(what) + "_2.fq", b.text);
  Fd fa, fb;
  CHECK(fa.open(pa, O_RDONLY) && fb.open(pb, O_RDONLY));
  for (int world = 1; world <= 5; world++) {
    const std::vector<uint64_t> ga = tentative(fa.get(), a.text.size(), world), gb = tentative(fb.get(), b.text.size(), world);
    const LineRanges la(world, ga.data()), lb(world, gb.data());
    CHECK(la.lines() == 4u * (uint64_t)n && lb.lines() == 4u * (uint64_t)n);
    CHECK(la.refusal(nullptr) == LineRanges::OK);
    const std::vector<uint64_t> K = la.first_records();
    CHECK(lb.refusal(&K) == LineRanges::OK);
    CHECK(K.size() == (size_t)world + 1 && K[0] == 0 && K[world] == (uint64_t)n);
    uint64_t end_a = 0, end_b = 0;  // where the rank before stopped
    for (int r = 0; r < world; r++) {
      CHECK(K[r] <= K[r + 1]);
      const uint64_t lo_a = la.offset_of_line(fa.get(), a.text.size(), 4 * K[r]), hi_a = la.offset_of_line(fa.get(), a.text.size(), 4 * K[r + 1]);
      const uint64_t lo_b = lb.offset_of_line(fb.get(), b.text.size(), 4 * K[r]), hi_b = lb.offset_of_line(fb.get(), b.text.size(), 4 * K[r + 1]);
      // the ranges follow one another without a gap, and each begins at the start of record K[r] -- in both mates
      CHECK(lo_a == end_a && lo_b == end_b);
      CHECK(lo_a == a.rec[K[r]] && hi_a == a.rec[K[r + 1]]);
      CHECK(lo_b == b.rec[K[r]] && hi_b == b.rec[K[r + 1]]);
      end_a = hi_a; end_b = hi_b;
    }
    CHECK(end_a == a.text.size() && end_b == b.text.size());
  }
}
static void check_cuts() {
  for (int n : {0, 1, 3, 37}) {
    char what[32];
    snprintf(what, sizeof what, "cuts%d", n);
    check_cuts_of(fastq(n, 20, 1), fastq(n, 33, 5), what);
  }
  // records of one size: the byte N-ths of the file are line starts themselves
  const Fastq eq = fastq(4, 10, 2, true);
  for (int i = 0; i <= 4; i++) CHECK(eq.rec[i] == (uint64_t)i * eq.rec[1]);
  check_cuts_of(eq, fastq(4, 17, 9), "cuts_even");
  {
    Fd f;
    CHECK(f.open(in_dir("cuts_even_1.fq"), O_RDONLY));
    CHECK(line_start(f.get(), eq.text.size(), 2, 1) == eq.rec[2]);
    CHECK(line_start(f.get(), eq.text.size(), 4, 3) == eq.rec[3]);
  }
  {  // count_newlines over more than one of its 64 MiB slices, between two offsets that are no multiples of anything
    std::string block(1u << 20, 'x');
    for (size_t i = 0; i < block.size(); i += 97) block[i] = '\n';
    const size_t blocks = 130, a = 12345, tail = 54321;
    const std::string path = in_dir("many_lines.txt");
    FILE *out = fopen(path.c_str(), "wb");
    CHECK(out);
    for (size_t i = 0; i < blocks; i++) CHECK(fwrite(block.data(), 1, block.size(), out) == block.size());
    fclose(out);
    const uint64_t per_block = (uint64_t)std::count(block.begin(), block.end(), '\n');
    const uint64_t want = blocks * per_block - (uint64_t)std::count(block.begin(), block.begin() + a, '\n') -
                          (uint64_t)std::count(block.end() - tail, block.end(), '\n');
    Fd f;
    CHECK(f.open(path, O_RDONLY));
    for (int threads : {1, 3, 16}) CHECK(count_newlines(f.get(), a, blocks * block.size() - tail, threads) == want);
    CHECK(count_newlines(f.get(), a, a, 3) == 0);
    unlink(path.c_str());
  }
  // the two refusals
  const std::string six = "@a\nAC\n+\nII\n@b\nGT\n";
  const Fastq three = fastq(3, 20, 1), four = fastq(4, 20, 1);
  Fd f6, f3, f4;
  CHECK(f6.open(put("six.fq", six), O_RDONLY) && f3.open(put("three.fq", three.text), O_RDONLY) && f4.open(put("four.fq", four.text), O_RDONLY));
  for (int world = 1; world <= 3; world++) {
    const std::vector<uint64_t> g6 = tentative(f6.get(), six.size(), world);
    const LineRanges l6(world, g6.data());
    CHECK(l6.lines() == 6 && l6.refusal(nullptr) == LineRanges::NOT_WHOLE_RECORDS);
    const std::vector<uint64_t> g3 = tentative(f3.get(), three.text.size(), world), g4 = tentative(f4.get(), four.text.size(), world);
    const LineRanges l3(world, g3.data()), l4(world, g4.data());
    const std::vector<uint64_t> K3 = l3.first_records();
    CHECK(l3.refusal(nullptr) == LineRanges::OK && l4.refusal(nullptr) == LineRanges::OK);
    CHECK(l4.refusal(&K3) == LineRanges::MATES_DIFFER && l3.refusal(&K3) == LineRanges::OK);
  }
}

// ---- place_share: every rank writes its share into one file --------------------------------------------------------------
static void check_place_share() {
  const uint32_t nb = 4;
  const int32_t cores[nb] = {7, -3, 11, 1 << 20};
  const std::string head = "HEAD!";
  for (int with_headers = 0; with_headers < 2; with_headers++)
    for (int world = 1; world <= 4; world++) {
      // bucket 2 is empty in the run, bucket 1 on the last rank of several
      std::vector<uint64_t> amount((size_t)world * nb);
      for (int r = 0; r < world; r++)
        for (uint32_t k = 0; k < nb; k++) amount[(size_t)r * nb + k] = k == 2 || (k == 1 && world > 1 && r == world - 1) ? 0 : (uint64_t)(r + 1) * (k + 2);
      auto unit = [](size_t k) { return (uint64_t)k + 1; };
      auto data_byte = [](int r, uint32_t k, uint64_t i) { return (uint8_t)(r * 64 + k * 16 + i % 16 + 1); };
      // a rank's own bytes: per bucket it has units in, (the 12 bytes of a header it does not write and) its units
      std::vector<Bytes> mine(world);
      for (int r = 0; r < world; r++)
        for (uint32_t k = 0; k < nb; k++) {
          const uint64_t n = amount[(size_t)r * nb + k] * unit(k);
          if (!n) continue;
          if (with_headers) mine[r].insert(mine[r].end(), 12, 0xEE);
          for (uint64_t i = 0; i < n; i++) mine[r].push_back(data_byte(r, k, i));
        }
      Bytes expect = bytes_of(head);
      for (uint32_t k = 0; k < nb; k++) {
        uint64_t all = 0;
        for (int r = 0; r < world; r++) all += amount[(size_t)r * nb + k];
        if (with_headers && all) {
          uint8_t hd[12];
          memcpy(hd, &cores[k], 4); memcpy(hd + 4, &all, 8);
          expect.insert(expect.end(), hd, hd + 12);
        }
        for (int r = 0; r < world; r++)
          for (uint64_t i = 0; i < amount[(size_t)r * nb + k] * unit(k); i++) expect.push_back(data_byte(r, k, i));
      }
      for (int reverse = 0; reverse < 2; reverse++) {
        const std::string path = in_dir("shares.bin");
        Fd f;
        CHECK(f.open(path, O_CREAT | O_TRUNC | O_WRONLY, 0644));
        for (int i = 0; i < world; i++) {
          const int r = reverse ? world - 1 - i : i;
          const Shares sh(amount.data(), nb, world, r);
          if (r == 0) pwrite_all(f.get(), head.data(), head.size(), 0);
          if (with_headers) place_share(f.get(), head.size(), mine[r].data(), sh, unit, cores, r == 0);
          else place_share(f.get(), head.size(), mine[r].data(), sh, unit);
        }
        f.release();
        CHECK(get(path) == expect);
      }
    }
}

// ---- MateSource ----------------------------------------------------------------------------------------------
static std::string read_all(MateSource &src, size_t cap) {
  std::string out;
  for (;;) {
    std::unique_ptr<char[]> piece(new char[cap]);  // (what a read writes is all it may write)
    const int64_t k = src.read(piece.get(), cap);
    CHECK(k >= 0 && (uint64_t)k <= cap);
    if (!k) return out;
    out.append(piece.get(), (size_t)k);
  }
}
static void check_mate_source() {
  const Fastq one = fastq(5, 12, 3), two = fastq(4, 12, 8);
  const std::string first = one.text.substr(0, one.text.size() - 1);  // no newline at its end
  const std::string joined = first + "\n" + two.text;
  const std::string p1 = put("join_1.fq", first), p2 = put("join_2.fq", two.text), p2z = put("join_2.fq.gz", gzip_of(two.text));
  CHECK(!is_gzip(p1) && is_gzip(p2z));
  for (const std::string &second : {p2, p2z}) {
    for (size_t cap : {(size_t)1, (size_t)7, joined.size() + 100}) {
      MateSource src;
      src.files = {p1, second};
      CHECK(read_all(src, cap) == joined);
    }
    // the sample holds at the end of the first file; what is read afterwards is everything, once
    MateSource src;
    src.files = {p1, second};
    src.fill_peek(1000, 4);
    CHECK(std::string(src.peek.begin(), src.peek.end()) == first + "\n");
    CHECK(read_all(src, 7) == joined);
  }
  {  // a sample smaller than the file stops reading ahead; the rest still arrives
    MateSource src;
    src.files = {p1, p2};
    src.fill_peek(2, 4);
    CHECK(src.peek.size() >= one.rec[2]);
    CHECK(read_all(src, 5) == joined);
  }
  // -i: whole pairs in every file
  const std::string p3 = put("odd.fq", fastq(3, 12, 1).text), p4 = put("even.fq", fastq(4, 12, 1).text);
  {
    MateSource src;
    src.files = {p3, p4};
    src.pair_lines = 8;
    char buf[64];
    int64_t k;
    while ((k = src.read(buf, sizeof buf)) > 0) {}
    CHECK(k == -1);
    CHECK(src.error.find("odd.fq holds an odd number of records (3)") != std::string::npos);
  }
  {
    MateSource src;
    src.files = {p4, p4};
    src.pair_lines = 8;
    const std::string four = fastq(4, 12, 1).text;
    CHECK(read_all(src, 64) == four + four && src.error.empty());
  }
  // sample_stats against a plain recount
  const Fastq f = fastq(9, 15, 4);
  for (int stride = 1; stride <= 2; stride++)
    for (int first_rec = 0; first_rec < stride; first_rec++)
      for (int sample : {1, 3, 100}) {
        int32_t want[128] = {0}, got[128] = {0};
        int want_len = 0, got_len = 0;
        for (int r = 0, taken = 0; r < 9 && taken < sample; r++) {
          if (r % stride != first_rec) continue;
          taken++;
          const std::string rec = f.text.substr(f.rec[r], f.rec[r + 1] - f.rec[r]);
          const std::string qual = rec.substr(rec.rfind('\n', rec.size() - 2) + 1, std::string::npos);
          for (size_t j = 0; j + 1 < qual.size(); j++) want[qual[j] & 127]++;
          want_len = (int)qual.size() - 1;
        }
        sample_stats(reinterpret_cast<const uint8_t *>(f.text.data()), f.text.size(), sample, got, got_len, stride, first_rec);
        CHECK(got_len == want_len && want_len == 15 && !memcmp(want, got, sizeof want));
      }
}

// ---- Fd, ArchiveFile --------------------------------------------------------------------------------------------
static void check_fd() {
  const std::string p = put("fd.bin", "0123456789");
  const int before = open_descriptors();
  {
    Fd a, b;
    CHECK(a.get() == -1 && !a.open(in_dir("not_there"), O_RDONLY) && a.get() == -1);
    CHECK(a.open(p, O_RDONLY) && a.get() >= 0);
    const int raw = a.get();
    b = std::move(a);
    CHECK(a.get() == -1 && b.get() == raw);
    Fd c(std::move(b));
    CHECK(b.get() == -1 && c.get() == raw && open_descriptors() == before + 1);
    CHECK(c.open(p, O_RDONLY) && open_descriptors() == before + 1);  // (the one it held went first)
    c.release();
    CHECK(c.get() == -1 && open_descriptors() == before);
    CHECK(c.open(p, O_RDONLY));
  }
  CHECK(open_descriptors() == before);
  {
    ArchiveFile plain, gz;
    plain.open(p);
    gz.open(put("fd.bin.gz", gzip_of("0123456789")));
    CHECK(!plain.gz && gz.gz);
    char buf[16];
    CHECK(ArchiveFile::read(&plain, buf, 3) == 3 && !memcmp(buf, "012", 3));
    CHECK(ArchiveFile::skip(&plain, 2) == 2 && ArchiveFile::read(&plain, buf, 16) == 5 && !memcmp(buf, "56789", 5));
    CHECK(ArchiveFile::skip(&plain, 4) == 0 && ArchiveFile::read(&plain, buf, 16) == 0);
    CHECK(ArchiveFile::skip(&gz, 2) == -1 && ArchiveFile::read(&gz, buf, 16) == 10 && !memcmp(buf, "0123456789", 10));
  }
  CHECK(open_descriptors() == before);
}

// ---- OutFile ----------------------------------------------------------------------------------------------
static void check_out_file() {
  for (size_t n : {(size_t)0, (size_t)1, OutFile::MEMBER, OutFile::MEMBER + 1}) {
    Bytes data(n);
    uint32_t x = 12345;
    for (size_t i = 0; i < n; i++) {  // the first half shrinks under deflate, the second hardly does
      x = x * 1664525u + 1013904223u;
      data[i] = i < n / 2 ? (uint8_t)"ACGT"[(i / 5) & 3] : (uint8_t)(x >> 24);
    }
    const std::string path = in_dir("out.gz");
    OutFile f;
    f.open(path, true);
    f.write(data.data(), n / 3);
    f.write(data.data() + n / 3, n - n / 3);
    f.close();
    const Bytes file = get(path);
    CHECK(file.size() >= 18 && file[0] == 0x1F && file[1] == 0x8B);  // (the empty case too is a gzip file)
    CHECK(gunzip_members(file) == data);
    OutFile plain;
    plain.open(path, false);
    plain.write(data);
    plain.close();
    CHECK(get(path) == data);
  }
}

// ---- the side files' headers ----------------------------------------------------------------------------------
static void check_side_files() {
  using namespace scalce_host;
  const std::string path = in_dir("side");
  CHECK(!side_file_present(path));
  OutFile f;
  f.open(path, false);
  side_file_header<LEN_HEADER_BYTES>(f, len_header_write, 300);
  side_file_header<ORDER_HEADER_BYTES>(f, order_header_write, (uint64_t)7);
  side_file_header<COMMENT_HEADER_BYTES>(f, comment_header_write, (uint32_t)13, (uint64_t)4);
  side_file_header<PLUS_HEADER_BYTES>(f, plus_header_write, (uint32_t)0, (uint64_t)5);
  side_file_header<EXCEPTION_HEADER_BYTES>(f, exception_header_write, (uint32_t)100, (uint64_t)3, (uint64_t)2);
  f.close();
  CHECK(side_file_present(path));
  Bytes want;  // the five headers, field by field: magic, int32 width, int32 parameter, the int64 counts
  auto header = [&](int32_t width, int32_t param, std::initializer_list<int64_t> counts) {
    want.insert(want.end(), {'s', 'c', 'a', 'l', 'c', 'e', '2', '2'});
    for (int32_t v : {width, param}) want.insert(want.end(), reinterpret_cast<uint8_t *>(&v), reinterpret_cast<uint8_t *>(&v) + 4);
    for (int64_t v : counts) want.insert(want.end(), reinterpret_cast<uint8_t *>(&v), reinterpret_cast<uint8_t *>(&v) + 8);
  };
  header(2, 300, {});
  header(4, 0, {7});
  header(0, 13, {4});
  header(0, 0, {5});
  header(8, 100, {3, 2});
  CHECK(want.size() == 16 + 24 + 24 + 24 + 32 && get(path) == want);
}

// ---- TextSink ----------------------------------------------------------------------------------------------
static void feed(TextSink &sink, const Fastq &f, int first, int n) {  // records first .. first + n as one window
  std::vector<uint64_t> roff(n + 1);
  for (int i = 0; i <= n; i++) roff[i] = f.rec[first + i] - f.rec[first];
  const Bytes text(f.text.begin() + f.rec[first], f.text.begin() + f.rec[first + n]);  // (a block of its own: a byte too far is seen)
  CHECK(TextSink::write(&sink, 0, (uint64_t)first, (uint64_t)n, text.data(), text.size(), roff.data()) == 0);
}
static void check_text_sink() {
  const Fastq f = fastq(9, 11, 6);
  auto records = [&](int a, int b) { return bytes_of(f.text.substr(f.rec[a], f.rec[b] - f.rec[a])); };
  for (int split : {4, 0}) {
    TextSink sink;
    sink.out = in_dir(split ? "parts" : "whole");
    sink.split = split;
    feed(sink, f, 0, 3);
    feed(sink, f, 3, 1);
    feed(sink, f, 4, 5);
    sink.finish(0);
    if (split) {
      CHECK(get(in_dir("parts.1_1.fastq")) == records(0, 4));
      CHECK(get(in_dir("parts.2_1.fastq")) == records(4, 8));
      CHECK(get(in_dir("parts.3_1.fastq")) == records(8, 9));
      CHECK(access(in_dir("parts.4_1.fastq").c_str(), F_OK) != 0 && sink.pm[0].files == 3);
    } else {
      CHECK(get(in_dir("whole_1.fastq")) == records(0, 9) && sink.pm[0].files == 1);
    }
  }
  for (int split : {4, 0}) {  // an archive without records: its one empty file
    TextSink sink;
    sink.out = in_dir(split ? "none_parts" : "none");
    sink.split = split;
    sink.finish(0);
    CHECK(get(in_dir(split ? "none_parts.1_1.fastq" : "none_1.fastq")).empty() && sink.pm[0].files == 1);
  }
}

int main(int argc, char **argv) {
  char made[] = "/tmp/cli_host_check_XXXXXX";
  g_dir = argc > 1 ? argv[1] : (mkdtemp(made) ? made : "");
  CHECK(!g_dir.empty());
  g_threads = 3;
  const int before = open_descriptors();
  check_cuts();
  check_mate_source();
  CHECK(open_descriptors() == before);  // every file of the two went with its owner
  check_fd();
  check_place_share();
  check_out_file();
  check_side_files();
  check_text_sink();
  CHECK(open_descriptors() == before);
  printf("cli_host_check: ok\n");
  return 0;
}
