// pcg_jit_cache.hpp -- the disk cache of run-time compiled code objects (pcg_abi_jit.hip: jit_module): its key digests, its
// directory and file format, and the checks that decide whether a file found there is loaded into the process.  Host only,
// libc and the standard library alone -- no HIP -- so that tools/hostcheck/host_code_check.cpp runs it under sanitizers.
#pragma once
#ifndef __HIPCC_RTC__

#include <dirent.h>
#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <cerrno>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iterator>
#include <map>
#include <mutex>
#include <string>
#include <vector>

namespace pcg {

inline uint64_t fnv1a(const std::string& s) {
  uint64_t h = 1469598103934665603ull;
  for (unsigned char ch : s) h = (h ^ ch) * 1099511628211ull;
  return h;
}

inline uint64_t fnv1a_seed(const std::string& s, uint64_t seed) {
  uint64_t h = 1469598103934665603ull ^ seed;
  for (unsigned char ch : s) h = (h ^ ch) * 1099511628211ull;
  return h;
}

// digest of the headers a run-time compilation will see: every *.hpp of the include directory and the ABI header
// next to it (../../include/pcgym_hip.h), by content.  Cached per directory for the life of the process.
inline std::string jit_header_digest(const char* inc_dir) {
  static std::map<std::string, std::string> memo;
  static std::mutex mu;
  std::lock_guard<std::mutex> lk(mu);
  auto it = memo.find(inc_dir);
  if (it != memo.end()) return it->second;
  std::vector<std::string> files;
  if (DIR* d = ::opendir(inc_dir)) {
    while (dirent* e = ::readdir(d)) {
      const std::string n = e->d_name;
      if (n.size() > 4 && n.compare(n.size() - 4, 4, ".hpp") == 0) files.push_back(std::string(inc_dir) + "/" + n);
    }
    ::closedir(d);
  }
  std::sort(files.begin(), files.end());
  files.push_back(std::string(inc_dir) + "/../../include/pcgym_hip.h");
  uint64_t h1 = 0, h2 = 0;
  for (const std::string& f : files) {
    std::ifstream in(f, std::ios::binary);
    const std::string body((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
    const std::string tag = f.substr(f.find_last_of('/') + 1) + ":" + std::to_string(body.size()) + ":";
    h1 = fnv1a_seed(tag + body, h1);
    h2 = fnv1a_seed(tag + body, h2 ^ 0x9E3779B97F4A7C15ull);
  }
  char hex[40];
  std::snprintf(hex, sizeof(hex), "%016llx%016llx", (unsigned long long)h1, (unsigned long long)h2);
  return memo[inc_dir] = hex;
}

// The disk cache lives in a directory only its owner can write: $PCG_JIT_CACHE, else $XDG_CACHE_HOME/pcgym_amd, else
// ~/.cache/pcgym_amd -- created with mkdir(2), mode 0700, no shell.  A directory (or file) that belongs to somebody
// else, or that group / others can write, is not used: code objects found there would run inside this process.
// Returns "" when there is no usable directory (the in-process cache still works).
inline bool jit_path_private(const std::string& p, bool want_dir) {
  struct stat st;
  if (::lstat(p.c_str(), &st) != 0) return false;
  if (want_dir ? !S_ISDIR(st.st_mode) : !S_ISREG(st.st_mode)) return false;
  return st.st_uid == ::geteuid() && (st.st_mode & (S_IWGRP | S_IWOTH)) == 0;
}
inline std::string jit_cache_dir() {
  std::string dir;
  if (const char* e = std::getenv("PCG_JIT_CACHE")) dir = e;
  else if (const char* x = std::getenv("XDG_CACHE_HOME")) dir = std::string(x) + "/pcgym_amd";
  else if (const char* h = std::getenv("HOME")) dir = std::string(h) + "/.cache/pcgym_amd";
  if (dir.empty() || dir[0] != '/') return std::string();
  for (size_t i = 1; i <= dir.size(); ++i)  // mkdir -p, without a shell
    if (i == dir.size() || dir[i] == '/') {
      const std::string part = dir.substr(0, i);
      if (::mkdir(part.c_str(), 0700) != 0 && errno != EEXIST) return std::string();
    }
  return jit_path_private(dir, true) ? dir : std::string();
}
// file = "PCGJIT2\n" nfn lowered names (one per line) code size, two 64-bit digests of (names + code) "\n" code
inline bool jit_cache_read(const std::string& path, int nfn, std::string* code, std::string* low) {
  if (!jit_path_private(path, false)) return false;
  std::ifstream in(path, std::ios::binary);
  std::string magic, line;
  if (!std::getline(in, magic) || magic != "PCGJIT2") return false;
  std::string all;
  for (int q = 0; q < nfn; ++q) {
    if (!std::getline(in, low[q]) || low[q].empty()) return false;
    all += low[q] + "\n";
  }
  unsigned long long sz = 0, d1 = 0, d2 = 0;
  if (!std::getline(in, line) || std::sscanf(line.c_str(), "%llu %llx %llx", &sz, &d1, &d2) != 3 || sz == 0 || sz > (1ull << 30))
    return false;
  std::string body((size_t)sz, '\0');
  in.read(&body[0], (std::streamsize)sz);
  if ((unsigned long long)in.gcount() != sz) return false;
  all += body;
  if (fnv1a(all) != d1 || fnv1a_seed(all, 0x9E3779B97F4A7C15ull) != d2) return false;  // truncated / corrupted / edited
  *code = std::move(body);
  return true;
}
inline void jit_cache_write(const std::string& path, int nfn, const std::string& code, const std::string* low) {
  // several processes (one per GPU) may compile the same source at once: a private temporary, complete and closed
  // before it appears under the final name; a write error never publishes a file
  const std::string tmp = path + "." + std::to_string((long long)getpid()) + ".tmp";
  const int fd = ::open(tmp.c_str(), O_WRONLY | O_CREAT | O_EXCL | O_NOFOLLOW, 0600);
  if (fd < 0) return;
  std::string all;
  for (int q = 0; q < nfn; ++q) all += low[q] + "\n";
  std::string head = "PCGJIT2\n" + all;
  all += code;
  char meta[96];
  std::snprintf(meta, sizeof(meta), "%llu %016llx %016llx\n", (unsigned long long)code.size(), (unsigned long long)fnv1a(all),
                (unsigned long long)fnv1a_seed(all, 0x9E3779B97F4A7C15ull));
  head += meta;
  bool ok = true;
  const std::string* parts[2] = {&head, &code};
  for (const std::string* part : parts) {
    size_t off = 0;
    while (ok && off < part->size()) {
      const ssize_t w = ::write(fd, part->data() + off, part->size() - off);
      if (w <= 0) ok = false;
      else off += (size_t)w;
    }
  }
  ok = (::close(fd) == 0) && ok;
  if (!ok || std::rename(tmp.c_str(), path.c_str()) != 0) ::unlink(tmp.c_str());
}

}  // namespace pcg
#endif  // !__HIPCC_RTC__
