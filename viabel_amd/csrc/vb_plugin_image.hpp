// vb_plugin_image.hpp — checks the bytes of a model plugin before HIP sees them.
//
// Host only and independent of HIP (tests/plugin_image_main.cc builds it alone, under the
// address and undefined-behaviour sanitizers).  The input is untrusted: every offset and
// size read from it is checked against the buffer before it is used, and every multi-byte
// field is read with memcpy (the buffer has no alignment).
//
// Accepted: a raw AMDGPU code object (ELF64, little-endian, e_machine 224, HSA OS ABI,
// ET_DYN, e_flags & 0xff == 0x4f: gfx950), or a __CLANG_OFFLOAD_BUNDLE__ whose entry
// "hipv4-amdgcn-amd-amdhsa--gfx950" is one -- what `hipcc --genco` writes with and without
// --no-gpu-bundle-output.  The symbol tables must define NAME (a function), NAME.kd (its
// 64-byte kernel descriptor) and NAME_launch (an object of at least 12 bytes with file
// contents), and the launch record must be valid (check_launch).
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstring>

namespace vbimg {

struct Image {
  uint64_t elf_off = 0, elf_size = 0;   // the code object inside the input
  bool bundled = false;
  int32_t launch[3] = {0, 0, 0};        // block, rows_per_block, dmax
};

constexpr char kBundleMagic[] = "__CLANG_OFFLOAD_BUNDLE__";   // 24 bytes
constexpr char kBundleId[] = "hipv4-amdgcn-amd-amdhsa--gfx950";
constexpr unsigned kMachineAmdgpu = 224, kMachGfx950 = 0x4f, kOsAbiHsa = 64;

namespace detail {

template <class T>
inline T rd(const unsigned char* p) {
  T v;
  std::memcpy(&v, p, sizeof v);
  return v;
}

// [off, off + len) lies inside [0, size)
inline bool inside(uint64_t off, uint64_t len, uint64_t size) {
  return off <= size && len <= size - off;
}

struct Sec {
  uint32_t name, type, link;
  uint64_t addr, off, size, entsize;
};

inline Sec sec_at(const unsigned char* sh) {
  Sec s;
  s.name = rd<uint32_t>(sh);
  s.type = rd<uint32_t>(sh + 4);
  s.addr = rd<uint64_t>(sh + 16);
  s.off = rd<uint64_t>(sh + 24);
  s.size = rd<uint64_t>(sh + 32);
  s.link = rd<uint32_t>(sh + 40);
  s.entsize = rd<uint64_t>(sh + 56);
  return s;
}

struct Sym {
  bool found = false;
  unsigned type = 0, shndx = 0;
  uint64_t value = 0, size = 0;
};

}  // namespace detail

// block a multiple of 64 in [64, 1024], rows_per_block >= 1, dmax >= 0
inline bool check_launch(const int32_t rec[3], char* err, size_t cap) {
  if (rec[0] < 64 || rec[0] > 1024 || rec[0] % 64 != 0) {
    std::snprintf(err, cap, "launch record: block %d is not a multiple of 64 in [64, 1024]", rec[0]);
    return false;
  }
  if (rec[1] < 1) {
    std::snprintf(err, cap, "launch record: rows_per_block %d is not >= 1", rec[1]);
    return false;
  }
  if (rec[2] < 0) {
    std::snprintf(err, cap, "launch record: dmax %d is negative", rec[2]);
    return false;
  }
  return true;
}

// The ELF at e[0 .. size): headers, section and segment bounds, the three symbols, the
// launch record.
inline bool check_elf(const unsigned char* e, uint64_t size, const char* kernel, Image* out,
                      char* err, size_t cap) {
  using namespace detail;
  if (size < 64) {
    std::snprintf(err, cap, "code object: %llu bytes are shorter than an ELF header",
                  (unsigned long long)size);
    return false;
  }
  if (std::memcmp(e, "\x7f" "ELF", 4) != 0) {
    std::snprintf(err, cap, "code object: no ELF magic");
    return false;
  }
  if (e[4] != 2 || e[5] != 1) {
    std::snprintf(err, cap, "code object: not a 64-bit little-endian ELF (class %d, data %d)", e[4], e[5]);
    return false;
  }
  const unsigned machine = rd<uint16_t>(e + 18), type = rd<uint16_t>(e + 16);
  if (machine != kMachineAmdgpu) {
    std::snprintf(err, cap, "code object: e_machine %u is not AMDGPU (224)", machine);
    return false;
  }
  if (e[7] != kOsAbiHsa) {
    std::snprintf(err, cap, "code object: OS ABI %d is not AMDGPU HSA (64)", e[7]);
    return false;
  }
  const uint32_t flags = rd<uint32_t>(e + 48);
  if ((flags & 0xff) != kMachGfx950) {
    std::snprintf(err, cap, "code object: built for another GPU (e_flags & 0xff = 0x%02x, gfx950 is 0x4f)",
                  flags & 0xff);
    return false;
  }
  if (type != 3) {
    std::snprintf(err, cap, "code object: e_type %u is not a linked (ET_DYN) code object", type);
    return false;
  }
  // program headers: every segment's file range lies inside the file
  const uint64_t phoff = rd<uint64_t>(e + 32);
  const unsigned phentsize = rd<uint16_t>(e + 54), phnum = rd<uint16_t>(e + 56);
  if (phnum) {
    if (phentsize < 56 || !inside(phoff, (uint64_t)phentsize * phnum, size)) {
      std::snprintf(err, cap, "code object: program header table lies outside the file (truncated?)");
      return false;
    }
    for (unsigned i = 0; i < phnum; ++i) {
      const unsigned char* ph = e + phoff + (uint64_t)i * phentsize;
      if (!inside(rd<uint64_t>(ph + 8), rd<uint64_t>(ph + 32), size)) {
        std::snprintf(err, cap, "code object: segment %u lies outside the file (truncated?)", i);
        return false;
      }
    }
  }
  // section headers
  const uint64_t shoff = rd<uint64_t>(e + 40);
  const unsigned shentsize = rd<uint16_t>(e + 58), shnum = rd<uint16_t>(e + 60);
  if (shoff == 0 || shnum == 0) {
    std::snprintf(err, cap, "code object: no section headers (no symbol table)");
    return false;
  }
  if (shentsize < 64 || !inside(shoff, (uint64_t)shentsize * shnum, size)) {
    std::snprintf(err, cap, "code object: section header table lies outside the file (truncated?)");
    return false;
  }
  auto sec = [&](unsigned i) { return sec_at(e + shoff + (uint64_t)i * shentsize); };
  for (unsigned i = 0; i < shnum; ++i) {
    const Sec s = sec(i);
    if (s.type != 0 && s.type != 8 /* NOBITS */ && !inside(s.off, s.size, size)) {
      std::snprintf(err, cap, "code object: section %u lies outside the file (truncated?)", i);
      return false;
    }
  }
  // the three symbols, from .symtab (2) or .dynsym (11)
  const size_t klen = std::strlen(kernel);
  Sym fn, kd, rec;
  for (unsigned i = 0; i < shnum; ++i) {
    const Sec s = sec(i);
    if (s.type != 2 && s.type != 11) continue;
    if (s.entsize != 24 || s.link >= shnum) {
      std::snprintf(err, cap, "code object: symbol table %u is malformed", i);
      return false;
    }
    const Sec st = sec(s.link);
    if (st.type != 3 /* STRTAB */) {
      std::snprintf(err, cap, "code object: symbol table %u has no string table", i);
      return false;
    }
    const uint64_t nsym = s.size / 24;
    for (uint64_t k = 0; k < nsym; ++k) {
      const unsigned char* sp = e + s.off + k * 24;
      const uint32_t noff = rd<uint32_t>(sp);
      if (noff >= st.size) continue;
      const char* name = reinterpret_cast<const char*>(e + st.off + noff);
      const uint64_t room = st.size - noff;   // bytes up to the table's end
      // the name must end inside the string table
      const void* nul = std::memchr(name, 0, (size_t)room);
      if (!nul) continue;
      const size_t nlen = (size_t)(static_cast<const char*>(nul) - name);
      Sym* dst = nullptr;
      if (nlen == klen && std::memcmp(name, kernel, klen) == 0) dst = &fn;
      else if (nlen == klen + 3 && std::memcmp(name, kernel, klen) == 0 &&
               std::memcmp(name + klen, ".kd", 3) == 0) dst = &kd;
      else if (nlen == klen + 7 && std::memcmp(name, kernel, klen) == 0 &&
               std::memcmp(name + klen, "_launch", 7) == 0) dst = &rec;
      if (!dst) continue;
      const unsigned shndx = rd<uint16_t>(sp + 6);
      if (shndx == 0) continue;   // undefined here
      dst->found = true;
      dst->type = sp[4] & 0xf;
      dst->shndx = shndx;
      dst->value = rd<uint64_t>(sp + 8);
      dst->size = rd<uint64_t>(sp + 16);
    }
  }
  if (!fn.found || fn.type != 2 /* FUNC */) {
    std::snprintf(err, cap, "code object: no kernel function '%.100s' in the symbol table", kernel);
    return false;
  }
  if (!kd.found || kd.type != 1 /* OBJECT */ || kd.size != 64) {
    std::snprintf(err, cap, "code object: no kernel descriptor '%.100s.kd' ('%.100s' is not a __global__ "
                  "function?)", kernel, kernel);
    return false;
  }
  if (!rec.found || rec.type != 1) {
    std::snprintf(err, cap, "code object: no launch record '%.100s_launch' in the symbol table", kernel);
    return false;
  }
  if (rec.size < 12) {
    std::snprintf(err, cap, "code object: launch record '%.100s_launch' holds %llu bytes, needs 12", kernel,
                  (unsigned long long)rec.size);
    return false;
  }
  if (rec.shndx >= shnum) {
    std::snprintf(err, cap, "code object: launch record '%.100s_launch' is in no section", kernel);
    return false;
  }
  const Sec rs = sec(rec.shndx);
  if (rs.type != 1 /* PROGBITS */ || rec.value < rs.addr || !inside(rec.value - rs.addr, 12, rs.size)) {
    std::snprintf(err, cap, "code object: launch record '%.100s_launch' has no initialised bytes in its "
                  "section", kernel);
    return false;
  }
  const unsigned char* rp = e + rs.off + (rec.value - rs.addr);   // inside the file: rs is
  for (int i = 0; i < 3; ++i) out->launch[i] = rd<int32_t>(rp + 4 * i);
  return check_launch(out->launch, err, cap);
}

// The whole check.  True: *out describes the code object; false: err holds one line.
inline bool check_image(const void* image, int64_t bytes, const char* kernel, Image* out, char* err,
                        size_t cap) {
  using namespace detail;
  Image img;
  if (!kernel || !kernel[0] || std::strlen(kernel) > 200) {
    std::snprintf(err, cap, "plugin image: the kernel name is empty or longer than 200 characters");
    return false;
  }
  if (!image || bytes <= 0) {
    std::snprintf(err, cap, "plugin image: empty input");
    return false;
  }
  const unsigned char* p = static_cast<const unsigned char*>(image);
  const uint64_t size = (uint64_t)bytes;
  if (size < 4) {
    std::snprintf(err, cap, "plugin image: %llu bytes are too short for a code object",
                  (unsigned long long)size);
    return false;
  }
  const size_t ml = sizeof kBundleMagic - 1;
  if (size >= ml && std::memcmp(p, kBundleMagic, ml) == 0) {
    if (size < ml + 8) {
      std::snprintf(err, cap, "offload bundle: truncated header");
      return false;
    }
    const uint64_t n = rd<uint64_t>(p + ml);
    uint64_t pos = ml + 8;
    bool found = false;
    const size_t idl = sizeof kBundleId - 1;
    for (uint64_t i = 0; i < n; ++i) {
      if (!inside(pos, 24, size)) {
        std::snprintf(err, cap, "offload bundle: entry table runs past the end (truncated?)");
        return false;
      }
      const uint64_t off = rd<uint64_t>(p + pos), len = rd<uint64_t>(p + pos + 8),
                     il = rd<uint64_t>(p + pos + 16);
      pos += 24;
      if (!inside(pos, il, size)) {
        std::snprintf(err, cap, "offload bundle: entry id runs past the end (truncated?)");
        return false;
      }
      if (!found && il == idl && std::memcmp(p + pos, kBundleId, idl) == 0) {
        if (!inside(off, len, size)) {
          std::snprintf(err, cap, "offload bundle: the gfx950 entry (offset %llu, %llu bytes) lies outside "
                        "the %llu-byte file", (unsigned long long)off, (unsigned long long)len,
                        (unsigned long long)size);
          return false;
        }
        img.elf_off = off;
        img.elf_size = len;
        found = true;
      }
      pos += il;
    }
    if (!found) {
      std::snprintf(err, cap, "offload bundle: no entry '%s'", kBundleId);
      return false;
    }
    img.bundled = true;
  } else {
    img.elf_off = 0;
    img.elf_size = size;
  }
  if (!check_elf(p + img.elf_off, img.elf_size, kernel, &img, err, cap)) return false;
  if (out) *out = img;
  return true;
}

}  // namespace vbimg
