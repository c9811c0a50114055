// Stand-alone driver of the host part of viabel_amd/csrc/vb_links.hpp for
// tests/test_links_host.py: no HIP, its own main.  Doubles travel as the hex of their
// bits.  Arguments, any number of:
//   h X                 prints lgamma_half_step(X)
//   c LIK NU SIGMA PHI  prints k0 k1 k2 k3 c_obs of link_consts
// The first line printed is kLog2Pi.
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "vb_links.hpp"

static_assert(!vbk::link_has_offset(0) && !vbk::link_has_offset(1) && !vbk::link_has_offset(2) &&
              vbk::link_has_offset(3) && vbk::link_has_offset(4), "the count likelihoods are 3 and 4");
static_assert(sizeof(vbk::LinkK) == 4 * sizeof(double), "four doubles in a kernel's argument block");

static double from_hex(const char* s) {
  const uint64_t u = std::strtoull(s, nullptr, 16);
  double d;
  std::memcpy(&d, &u, sizeof d);
  return d;
}

static void put(double d, const char* end) {
  uint64_t u;
  std::memcpy(&u, &d, sizeof u);
  std::printf("%016" PRIx64 "%s", u, end);
}

int main(int argc, char** argv) {
  put(vbk::kLog2Pi, "\n");
  for (int i = 1; i < argc;) {
    if (argv[i][0] == 'h' && i + 1 < argc) {
      put(vbk::lgamma_half_step(from_hex(argv[i + 1])), "\n");
      i += 2;
    } else if (argv[i][0] == 'c' && i + 4 < argc) {
      vbk::LinkK k;
      const double c = vbk::link_consts(std::atoi(argv[i + 1]), from_hex(argv[i + 2]),
                                        from_hex(argv[i + 3]), from_hex(argv[i + 4]), &k);
      put(k.k0, " ");
      put(k.k1, " ");
      put(k.k2, " ");
      put(k.k3, " ");
      put(c, "\n");
      i += 5;
    } else {
      std::fprintf(stderr, "bad argument %s\n", argv[i]);
      return 2;
    }
  }
  return 0;
}
