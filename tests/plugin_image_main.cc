// plugin_image_main.cc — runs the plugin image checker (viabel_amd/csrc/vb_plugin_image.hpp)
// alone, as its own process, so that tests/test_plugin_host.py can build it under the
// address and undefined-behaviour sanitizers: it includes nothing else of the library and
// needs no GPU.  Arguments are triples MODE KERNEL PATH:
//   ok     the file must pass the check
//   bad    the file must be refused with a message
//   trunc  every prefix of the file whose length is a multiple of 512 (and below the
//          file's) must be refused
// Each image is copied into a heap block of exactly its size, so a read past the end is
// a sanitizer report.  Exit status 0: everything as expected.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "vb_plugin_image.hpp"

static bool check_exact(const std::vector<unsigned char>& src, size_t len, const char* kernel,
                        char* err, size_t cap) {
  unsigned char* buf = static_cast<unsigned char*>(std::malloc(len ? len : 1));
  if (!buf) std::abort();
  if (len) std::memcpy(buf, src.data(), len);
  vbimg::Image img;
  err[0] = 0;
  const bool ok = vbimg::check_image(len ? buf : nullptr, (long long)len, kernel, &img, err, cap);
  std::free(buf);
  return ok;
}

int main(int argc, char** argv) {
  if (argc < 4 || (argc - 1) % 3 != 0) {
    std::fprintf(stderr, "usage: %s (ok|bad|trunc KERNEL PATH)...\n", argv[0]);
    return 2;
  }
  int failures = 0;
  for (int i = 1; i + 2 < argc; i += 3) {
    const std::string mode = argv[i];
    const char* kernel = argv[i + 1];
    const char* path = argv[i + 2];
    std::vector<unsigned char> bytes;
    if (FILE* f = std::fopen(path, "rb")) {
      unsigned char chunk[4096];
      size_t n;
      while ((n = std::fread(chunk, 1, sizeof chunk, f)) > 0) bytes.insert(bytes.end(), chunk, chunk + n);
      std::fclose(f);
    } else {
      std::fprintf(stderr, "cannot open %s\n", path);
      return 2;
    }
    char err[400];
    if (mode == "trunc") {
      int refused = 0;
      for (size_t len = 512; len < bytes.size(); len += 512) {
        if (check_exact(bytes, len, kernel, err, sizeof err) || !err[0]) {
          std::printf("FAIL trunc %s at %zu: accepted\n", path, len);
          ++failures;
        } else {
          ++refused;
        }
      }
      std::printf("trunc %s: %d prefixes refused\n", path, refused);
      continue;
    }
    const bool ok = check_exact(bytes, bytes.size(), kernel, err, sizeof err);
    const bool want = mode == "ok";
    if (ok != want || (!ok && !err[0])) {
      std::printf("FAIL %s %s (%s): %s\n", mode.c_str(), path, kernel, ok ? "accepted" : err);
      ++failures;
    } else {
      std::printf("%s %s (%s)%s%s\n", mode.c_str(), path, kernel, ok ? "" : ": ", ok ? "" : err);
    }
  }
  return failures ? 1 : 0;
}
