// host_code_check.cpp -- the device-free host code of the library, compiled for the HOST on its own: the policy block packers
// (pcg_policy_pack.hpp), whose layout is a contract with four kernel families, and the disk cache of run-time compiled code
// objects (pcg_jit_cache.hpp), which decides whether a file found on disk is loaded into the process.
//   * packing: every shape of n_hidden x n_in x n_out x widths below, both element types -- each element at the index the
//     kernel headers document, every other element behind the header exactly zero, sizes a function of the shape alone;
//   * cache file: a round trip, and every kind of file or directory that must be refused.
// Exits non-zero at the first failed check; the last line of a clean run states the shape count.
// Build and run: tools/hostcheck/run.sh (sanitizer builds, g++ / the ROCm clang++), tests/test_host_code_check.py (plain build).
// No GPU, no HIP runtime.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../pc-gym_amd/csrc/pcg_jit_cache.hpp"
#include "../../pc-gym_amd/csrc/pcg_policy_pack.hpp"

using namespace pcg;

#define CHECK(cond)                                                          \
  do {                                                                       \
    if (!(cond)) {                                                           \
      std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      std::exit(1);                                                          \
    }                                                                        \
  } while (0)

// ---- packing ------------------------------------------------------------------------------------------------------------
constexpr int HDR = (int)(sizeof(PolicyDev) / sizeof(double));  // the header, in doubles
static int up(int n, int m) { return (n + m - 1) / m * m; }

// a cfg of one shape with `members` member-major sets of distinct non-zero weights and biases (storage in `store`)
struct Net {
  pcg_policy_cfg cfg;
  std::vector<double> W[3], b[3];
};
static void fill(Net* n, int n_hidden, int n_in, int n_out, int w0, int w1, int members, double salt) {
  pcg_policy_cfg& c = n->cfg;
  c = pcg_policy_cfg();
  c.n_in = n_in; c.n_out = n_out; c.n_hidden = n_hidden;
  c.width[0] = w0; c.width[1] = w1;
  c.activation = PCG_ACT_TANH;
  c.out_map = PCG_POL_CLIP;
  c.out_low = -1.0 / 3.0 - salt; c.out_high = 2.0 / 3.0 + salt;  // (not float32 values: the rounded box differs)
  int ctr = 0;
  auto next = [&] { ++ctr; return (ctr * 1e-3 + 1.0 / 3.0 + salt) * ((ctr & 1) ? 1.0 : -1.0); };
  for (int l = 0; l <= n_hidden; ++l) {
    int rows, cols;
    policy_layer_dims(&c, l, &rows, &cols);
    n->W[l].resize((size_t)members * rows * cols);
    n->b[l].resize((size_t)members * rows);
    for (double& v : n->W[l]) v = next();
    for (double& v : n->b[l]) v = next();
    c.W[l] = n->W[l].data();
    c.b[l] = n->b[l].data();
  }
}

// element i behind the header of a block, as the kernels of its dtype read it
static double elem(const std::vector<double>& blob, int dtype, size_t i) {
  if (dtype == PCG_POL_F32) {
    CHECK(i < (blob.size() - HDR) * 2);
    float f;
    std::memcpy(&f, reinterpret_cast<const char*>(blob.data() + HDR) + 4 * i, 4);
    return (double)f;
  }
  CHECK(i < blob.size() - HDR);
  return blob[HDR + i];
}

// the flat parameter j of a member -> its element offset from the block's start: pcg_pop_search.hpp's pop_param_offset(_f32)
static int flat_offset(const PopLayout& L, int j) {
  int l = 0;
  if (L.nl > 1 && j >= L.start[1]) l = 1;
  if (L.nl > 2 && j >= L.start[2]) l = 2;
  const int local = j - L.start[l], cols = L.cols[l], nw = L.rows[l] * cols;
  if (local >= nw) return L.offb[l] + (local - nw);
  const int r = local / cols, k = local - r * cols;
  return L.f32 ? L.offW[l] + ((r >> 1) * L.ld[l] + k) * 2 + (r & 1) : L.offW[l] + r * L.ld[l] + k;
}

static void check_shape(int n_hidden, int n_in, int n_out, int w0, int w1) {
  Net net, other;
  fill(&net, n_hidden, n_in, n_out, w0, w1, 1, 0.0);
  fill(&other, n_hidden, n_in, n_out, w0, w1, 1, 0.125);
  const pcg_policy_cfg& c = net.cfg;
  CHECK(policy_validate(&c) == PCG_OK);
  int ld64[3] = {0, 0, 0};
  for (int dtype : {PCG_POL_F64, PCG_POL_F32}) {
    const bool f32 = dtype == PCG_POL_F32;
    int rc = -99;
    const std::vector<double> blob = pack_policy(&c, dtype, &rc);
    CHECK(rc == PCG_OK);
    PolicyDev h;
    CHECK(blob.size() > (size_t)HDR);
    std::memcpy(&h, blob.data(), sizeof(h));
    CHECK(h.n_in == n_in && h.n_out == n_out && h.n_hidden == n_hidden && h.act == c.activation && h.out_map == c.out_map);
    CHECK(h.w[0] == (n_hidden > 0 ? w0 : 0) && h.w[1] == (n_hidden > 1 ? w1 : 0));
    CHECK(h.out_lo == (f32 ? (double)(float)c.out_low : c.out_low) && h.out_hi == (f32 ? (double)(float)c.out_high : c.out_high));
    if (f32) CHECK(h.out_lo != c.out_low && h.out_hi != c.out_high);
    // the documented layout, restated: layer after layer, matrix then bias, padded rows x padded columns
    size_t off = 0, written = 0;
    for (int l = 0; l <= n_hidden; ++l) {
      int rows, cols;
      policy_layer_dims(&c, l, &rows, &cols);
      const int prow = l == n_hidden ? (f32 ? POL32_OR : PCG_MAX_NA) : up(rows, l == 0 ? POL_HB : POL_SB);
      const int ld = l == 0 ? up(cols, POL_IB) : up(cols, l == 1 ? POL_HB : POL_SB);
      CHECK(h.ld[l] == ld && h.offW[l] == (int32_t)off);
      if (!f32) ld64[l] = h.ld[l];
      CHECK(h.ld[l] == ld64[l]);  // ld agrees between the two forms
      for (int r = 0; r < rows; ++r)
        for (int k = 0; k < cols; ++k) {
          const double v = c.W[l][(size_t)r * cols + k];
          const size_t at = f32 ? ((size_t)(r / 2) * ld + k) * 2 + (r & 1) : (size_t)r * ld + k;
          CHECK(elem(blob, dtype, off + at) == (f32 ? (double)(float)v : v));
          ++written;
        }
      off += (size_t)prow * ld;
      CHECK(h.offb[l] == (int32_t)off);
      for (int r = 0; r < rows; ++r) {
        CHECK(elem(blob, dtype, off + r) == (f32 ? (double)(float)c.b[l][r] : c.b[l][r]));
        ++written;
      }
      off += (size_t)prow;
    }
    // the block's size: the data and its slack (16 doubles; 32 floats, rounded up to whole doubles), nothing else
    CHECK(blob.size() == (size_t)HDR + (f32 ? (off + 32 + 1) / 2 : off + 16));
    // all padding and slack is exactly zero: as many non-zero elements behind the header as values written
    const size_t total = (blob.size() - HDR) * (f32 ? 2 : 1);
    size_t nonzero = 0;
    for (size_t i = 0; i < total; ++i) nonzero += elem(blob, dtype, i) != 0.0;
    CHECK(nonzero == written);
    // the size is a function of the shape alone
    const std::vector<double> blob2 = pack_policy(&other.cfg, dtype, &rc);
    CHECK(rc == PCG_OK && blob2.size() == blob.size());
    // pop_layout of the packed member: the flat order against the block, the header counted in the block's elements
    const PopLayout L = pop_layout(&c, blob.data(), dtype);
    const int hdr = f32 ? 2 * HDR : HDR;
    CHECK(L.f32 == (f32 ? 1 : 0) && L.nl == n_hidden + 1 && L.n == (int)written && L.start[L.nl] == L.n);
    int j = 0;
    for (int l = 0; l <= n_hidden; ++l) {
      int rows, cols;
      policy_layer_dims(&c, l, &rows, &cols);
      CHECK(L.start[l] == j && L.rows[l] == rows && L.cols[l] == cols && L.ld[l] == h.ld[l]);
      CHECK(L.offW[l] == hdr + h.offW[l] && L.offb[l] == hdr + h.offb[l]);
      for (int i = 0; i < rows * cols; ++i, ++j) CHECK(elem(blob, dtype, (size_t)(flat_offset(L, j) - hdr)) == (f32 ? (double)(float)c.W[l][i] : c.W[l][i]));
      for (int r = 0; r < rows; ++r, ++j) CHECK(elem(blob, dtype, (size_t)(flat_offset(L, j) - hdr)) == (f32 ? (double)(float)c.b[l][r] : c.b[l][r]));
    }
    CHECK(j == L.n);
  }
}

static void check_refusals_and_pop() {
  int rc;
  Net net;
  // a weight, then a clip bound, that is finite in fp64 and not after rounding to float32
  fill(&net, 1, 3, 2, 5, 0, 1, 0.0);
  net.W[0][4] = 1e39;
  CHECK(policy_validate(&net.cfg) == PCG_OK);
  (void)pack_policy(&net.cfg, PCG_POL_F64, &rc);
  CHECK(rc == PCG_OK);
  (void)pack_policy(&net.cfg, PCG_POL_F32, &rc);
  CHECK(rc == PCG_E_VALUE);
  fill(&net, 1, 3, 2, 5, 0, 1, 0.0);
  net.cfg.out_high = 1e39;
  CHECK(policy_validate(&net.cfg) == PCG_OK);
  (void)pack_policy(&net.cfg, PCG_POL_F64, &rc);
  CHECK(rc == PCG_OK);
  (void)pack_policy(&net.cfg, PCG_POL_F32, &rc);
  CHECK(rc == PCG_E_VALUE);
  // three members: their blocks are the three single packs, back to back
  fill(&net, 2, 5, 2, 5, 63, 3, 0.0);
  CHECK(pop_validate(&net.cfg, 3) == PCG_OK);
  CHECK(pop_validate(&net.cfg, 0) == PCG_E_DIM && pop_validate(nullptr, 3) == PCG_E_NULL);
  for (int dtype : {PCG_POL_F64, PCG_POL_F32}) {
    size_t member = 0;
    const std::vector<double> all = pack_pop(&net.cfg, 3, dtype, &member, &rc);
    CHECK(rc == PCG_OK);
    std::vector<double> cat;
    for (int m = 0; m < 3; ++m) {
      const pcg_policy_cfg one = pop_member_cfg(&net.cfg, m);
      const std::vector<double> blob = pack_policy(&one, dtype, &rc);
      CHECK(rc == PCG_OK && blob.size() == member);
      cat.insert(cat.end(), blob.begin(), blob.end());
    }
    CHECK(all.size() == cat.size() && std::memcmp(all.data(), cat.data(), sizeof(double) * all.size()) == 0);
  }
}

static int check_packing() {
  const int ins[] = {1, 3, 4, 5, PCG_MAX_NOBS}, outs[] = {1, 2, PCG_MAX_NA}, widths[] = {1, 5, 8, 63, 64};
  int shapes = 0;
  for (int nh = 0; nh <= 2; ++nh)
    for (int n_in : ins)
      for (int n_out : outs)
        for (int w0 : widths) {
          for (int w1 : widths) {
            check_shape(nh, n_in, n_out, w0, w1);
            ++shapes;
            if (nh < 2) break;  // (the second width is ignored)
          }
          if (nh < 1) break;
        }
  check_refusals_and_pop();
  return shapes;
}

// ---- cache file ---------------------------------------------------------------------------------------------------------
static std::string slurp(const std::string& path) {
  std::ifstream in(path, std::ios::binary);
  return std::string((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
}
static void spit(const std::string& path, const std::string& body, mode_t mode = 0600) {
  const int fd = ::open(path.c_str(), O_WRONLY | O_CREAT | O_TRUNC, mode);
  CHECK(fd >= 0);
  CHECK(::write(fd, body.data(), body.size()) == (ssize_t)body.size());
  CHECK(::fchmod(fd, mode) == 0 && ::close(fd) == 0);  // (whatever the umask)
}
// the read must fail and load nothing
static void refused(const std::string& path, int nfn) {
  std::string code, low[4];
  CHECK(!jit_cache_read(path, nfn, &code, low));
  CHECK(code.empty());
}

static int check_cache() {
  char tmpl[] = "/tmp/pcg_host_check_XXXXXX";
  CHECK(::mkdtemp(tmpl) != nullptr);  // (created 0700)
  const std::string dir = tmpl, good = dir + "/good.pco";
  const std::string names[3] = {"_ZN3pcg11step_kernelILi0EEEvNS_8StepArgsE", "k1", "k2"};
  std::string code = "\x7f" "ELF";
  code += std::string("a\nb\0c\n\0\0", 8);
  for (int i = 0; i < 300; ++i) code.push_back((char)(i * 7));
  jit_cache_write(good, 3, code, names);
  {
    std::string got, low[3];
    CHECK(jit_cache_read(good, 3, &got, low));
    CHECK(got == code && low[0] == names[0] && low[1] == names[1] && low[2] == names[2]);
  }
  int cases = 1;
  const std::string file = slurp(good);
  CHECK(file.size() > code.size() && file.compare(file.size() - code.size(), code.size(), code) == 0);
  auto bad = [&](const char* name, const std::string& body, mode_t mode = 0600) {
    const std::string path = dir + "/" + name;
    spit(path, body, mode);
    refused(path, 3);
    ++cases;
  };
  refused(good, 2);  // a wrong nfn, either way
  refused(good, 4);
  cases += 2;
  std::string flipped = file;
  flipped[file.size() - code.size() / 2] ^= 0x01;
  bad("flipped.pco", flipped);
  bad("truncated.pco", file.substr(0, file.size() - 5));
  {  // a size line above 2^30 (the digests as written: the size alone refuses it)
    const size_t body = file.size() - code.size(), line = file.rfind('\n', body - 2) + 1, sp = file.find(' ', line);
    bad("huge.pco", file.substr(0, line) + "1073741825" + file.substr(sp));
  }
  bad("magic.pco", "PCGJIT1" + file.substr(7));
  bad("groupw.pco", file, 0620);
  {
    const std::string link = dir + "/link.pco";
    CHECK(::symlink(good.c_str(), link.c_str()) == 0);
    refused(link, 3);
    ++cases;
  }
  // the directory: an absolute path of one's own that nobody else can write, created 0700 where missing
  const std::string sub = dir + "/cache/pcgym";
  CHECK(::setenv("PCG_JIT_CACHE", sub.c_str(), 1) == 0 && jit_cache_dir() == sub && jit_path_private(sub, true));
  CHECK(::setenv("PCG_JIT_CACHE", "relative/cache", 1) == 0 && jit_cache_dir().empty());
  CHECK(::chmod(sub.c_str(), 0770) == 0 && ::setenv("PCG_JIT_CACHE", sub.c_str(), 1) == 0 && jit_cache_dir().empty());
  cases += 3;
  for (const char* n : {"good.pco", "flipped.pco", "truncated.pco", "huge.pco", "magic.pco", "groupw.pco", "link.pco"})
    (void)::unlink((dir + "/" + n).c_str());
  (void)::rmdir(sub.c_str());
  (void)::rmdir((dir + "/cache").c_str());
  (void)::rmdir(dir.c_str());
  return cases;
}

int main() {
  const int cases = check_cache();
  const int shapes = check_packing();
  std::printf("host_code_check ok: %d cache cases, %d shapes x 2 dtypes packed\n", cases, shapes);
  return 0;
}
