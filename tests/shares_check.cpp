// Stand-alone check of csrc/mf_shares.hpp (tests/test_host_cpu.py builds it with -fsanitize=address,undefined and runs it):
// the scratch carver with a null base (the size query) and with a real buffer, over the layouts of the units that carve, and
// the invariants of share_of.  It includes nothing else of the library.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "mf_shares.hpp"

using mf::Carver;

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { ++failures; std::printf("FAILED %s: ", #cond); std::printf(__VA_ARGS__); std::printf("\n"); } } while (0)

struct Field { long long size, count, align; };

template <class T>
static void take_one(Carver& c, const Field& f, std::vector<char*>& got) { got.push_back(reinterpret_cast<char*>(c.take<T>(f.count, f.align))); }

static void take(Carver& c, const Field& f, std::vector<char*>& got) {
  switch (f.size) {
    case 1: take_one<unsigned char>(c, f, got); break;
    case 4: take_one<int>(c, f, got); break;
    case 8: take_one<long long>(c, f, got); break;
    default: { struct Row { float v[4]; }; take_one<Row>(c, f, got); }      // 16: a position row
  }
}

// the layout carved from null and from a real buffer: the same size, every pointer at base + the offset counted here
static void check_layout(const char* name, const std::vector<Field>& fields) {
  std::vector<long long> want;
  long long at = 0;
  for (const Field& f : fields) { want.push_back(at); at += (f.size * f.count + f.align - 1) / f.align * f.align; }
  std::vector<char*> got;
  Carver sizing(nullptr);
  for (const Field& f : fields) take(sizing, f, got);
  CHECK(sizing.bytes() == at, "%s: %lld bytes from null, %lld counted", name, sizing.bytes(), at);
  if (at > (64LL << 20)) return;                                            // the large shapes: sizes alone
  char* buf = static_cast<char*>(std::malloc((size_t)at + 1));
  Carver real(buf);
  got.clear();
  for (const Field& f : fields) take(real, f, got);
  CHECK(real.bytes() == at, "%s: %lld bytes from a buffer, %lld counted", name, real.bytes(), at);
  for (size_t i = 0; i < fields.size(); ++i) {
    CHECK(got[i] == buf + want[i], "%s: field %zu at %lld, not %lld", name, i, (long long)(got[i] - buf), want[i]);
    const long long n = fields[i].size * fields[i].count;
    if (n > 0) std::memset(got[i], 0x5a, (size_t)n);                        // inside the buffer, or the address sanitizer stops here
  }
  std::free(buf);
}

int main() {
  const long long kTile = 256, kCompactTile = 4096, kBlocks = 2048, kCompactBlocks = 1024;
  const long long edges[] = {0, 1, kTile - 1, kTile, kTile + 1, kCompactTile - 1, kCompactTile, kCompactTile + 1,
                             kBlocks * kTile - 1, kBlocks * kTile, kBlocks * kTile + 1,
                             kCompactBlocks * kCompactTile - 1, kCompactBlocks * kCompactTile, kCompactBlocks * kCompactTile + 1};
  for (const long long n : edges) {
    const struct { int tile, max_blocks; } plans[] = {{(int)kTile, (int)kBlocks}, {(int)kCompactTile, (int)kCompactBlocks}, {64, 1}, {256, 3}};
    for (const auto& pl : plans) {
      const mf::Share s = mf::share_of(n, pl.tile, pl.max_blocks);
      CHECK(s.per > 0 && s.per % pl.tile == 0, "n=%lld tile=%d: per=%lld", n, pl.tile, s.per);
      CHECK(s.nblocks >= 0 && s.nblocks <= pl.max_blocks, "n=%lld: nblocks=%d of %d", n, s.nblocks, pl.max_blocks);
      CHECK((n == 0) == (s.nblocks == 0), "n=%lld: nblocks=%d", n, s.nblocks);
      if (n > 0) CHECK((s.nblocks - 1) * s.per < n && n <= s.nblocks * s.per, "n=%lld: %d shares of %lld", n, s.nblocks, s.per);
      const long long tiles = (n + pl.tile - 1) / pl.tile, div = (long long)pl.tile * pl.max_blocks;
      if (n > 0) CHECK(s.per == (n + div - 1) / div * pl.tile, "n=%lld: per=%lld", n, s.per);
      if (tiles <= pl.max_blocks) CHECK(s.per == pl.tile && s.nblocks == tiles, "n=%lld: one tile each", n);
    }
    const long long V = n, T = 2 * n + 1, W = (n + 31) / 32;
    const long long compact = 8 * mf::share_of(V > T ? V : T, (int)kCompactTile, (int)kCompactBlocks).nblocks;
    check_layout("component table", {{4, V, 16}, {4, V, 16}, {1, V, 16}, {8, 1, 16}, {1, compact, 16}});
    check_layout("component filter", {{1, V, 16}, {1, V, 16}, {1, T, 16}, {4, V, 16}, {8, 1, 16}, {1, compact, 16}});
    check_layout("simplify", {{4, V, 16}, {1, T, 16}, {4, W, 16}, {4, W, 16}, {8, kBlocks, 16}, {8, kBlocks, 16}, {4, 2 * T, 16}});
    check_layout("rings", {{4, 4, 16}, {4, V, 16}, {4, V + 1, 16}, {4, V, 16}, {8, kBlocks, 16}, {4, V < 7 ? V : 7, 16}, {4, 6 * T, 16}});
    check_layout("smooth", {{16, V, 16}, {16, V, 16}, {4, V + 1, 16}, {4, 6 * V, 16}});
    check_layout("regions", {{4, n, 16}, {4, n, 16}, {8, 3, 16}, {8, kBlocks, 16}});
    const long long nb = (n + 1023) / 1024;
    check_layout("marching cubes", {{8, 2 * nb, 16}, {4, 2 * nb, 8}, {4, n, 4}});
    check_layout("dilation", {{4, n, 16}, {4, n, 16}, {8, (n + 255) / 256, 8}});
  }
  CHECK(mf::align_up(0, 16) == 0 && mf::align_up(1, 16) == 16 && mf::align_up(16, 16) == 16 && mf::align_up(17, 8) == 24, "align_up");
  CHECK(mf::kIndexLimit == 2147483648LL, "kIndexLimit");
  if (failures) { std::printf("%d checks failed\n", failures); return 1; }
  std::printf("shares ok\n");
  return 0;
}
