// Stand-alone CPU test of the chunk plan and the step rule of the GBDT forest walk (gbdt_walk_map.hpp):
// for every forest below it runs gbdt_predict.hip's block as plain loops - the tile's bytes into an
// exactly sized LDS image, the chunk loop over windows of tree_off, the staging of every chunk, the walk
// of every row - through the header's functions, and checks invariants W1 .. W4 of the header.  Built
// by tests/test_gbdt_walk_map_cpu.py with -fsanitize=address,undefined (every array is an exactly
// sized heap array, so an access past one is an error).  Prints OK.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "gbdt_walk_map.hpp"
#define MAP_TEST_SUBJECT f.name
#include "test_map_common.hpp"

namespace gw = mp4x::gbdt_walk;

struct Forest {
  const char* name;
  std::vector<gw::Node> nodes;
  std::vector<int32_t> off;      // T + 1 entries
  int steps;
};

static int bin_of(int64_t r, int64_t f) { return (int)(((uint64_t)(r * 31 + f * 7 + 3) * 2654435761u >> 9) & 255); }
static double value_of(int64_t i) { return (double)((i * 37) % 101) - 50.0 + (i % 3 ? 1e-300 : 1e18); }

// A full binary tree of `depth` levels below the root, features and thresholds varied by node.
static void add_tree(Forest& f, int depth, int64_t F) {
  const int32_t size = (1 << (depth + 1)) - 1;
  for (int32_t i = 0; i < size; ++i) {
    const bool inner = 2 * i + 2 < size;
    f.nodes.push_back(inner ? gw::Node{(int32_t)((i * 5 + 1) % F), (int32_t)((i * 53) % 255), 2 * i + 1, 2 * i + 2}
                            : gw::Node{-1, -1, -1, -1});
  }
  f.off.push_back((int32_t)f.nodes.size());
}
// A chain of `size` nodes: every row goes down one side, a path of size - 1 edges.
static void add_chain(Forest& f, int32_t size) {
  for (int32_t i = 0; i < size; ++i)
    f.nodes.push_back(i + 1 < size ? gw::Node{0, i % 2 ? 255 : -1, i + 1, i + 1} : gw::Node{-1, 0, -1, -1});
  f.off.push_back((int32_t)f.nodes.size());
}

// The definition, written out: o by its own loop, the inner test spelled again.
static void define(const Forest& f, int64_t n, int64_t F, std::vector<double>& pred, std::vector<int32_t>& leaf) {
  const int64_t T = (int64_t)f.off.size() - 1, N = (int64_t)f.nodes.size();
  int64_t lo = 0;
  for (int64_t t = 0; t < T; ++t) {
    int64_t hi = f.off[t + 1] < N ? f.off[t + 1] : N;
    if (hi < lo) hi = lo;
    const int64_t size = hi - lo;
    for (int64_t r = 0; r < n; ++r) {
      int64_t j = 0;
      for (int s = 0; s < f.steps && size > 0; ++s) {
        const gw::Node& nd = f.nodes[(size_t)(lo + j)];
        if (nd.feature < 0 || nd.feature >= F || nd.left < 0 || nd.left >= size || nd.right < 0 || nd.right >= size) continue;
        j = bin_of(r, nd.feature) > nd.threshold ? nd.right : nd.left;
      }
      if (size > 0) pred[(size_t)r] += value_of(lo + j);
      leaf[(size_t)(r * T + t)] = size > 0 ? (int32_t)j : -1;
    }
    lo = hi;
  }
}

static void run(const Forest& f, int64_t n, int64_t F, uint64_t base) {
  const int64_t T = (int64_t)f.off.size() - 1, N = (int64_t)f.nodes.size();
  CHECK(f.steps >= 0 && f.steps <= gw::kMaxSteps && N < gw::kMaxRows && F >= 1, "limits");
  std::vector<double> want((size_t)n, 0.0), got((size_t)n, 0.0);
  std::vector<int32_t> want_leaf((size_t)(n * T), -7), got_leaf((size_t)(n * T), -7);
  define(f, n, F, want, want_leaf);
  int32_t* off = (int32_t*)std::malloc((size_t)(T + 1) * sizeof(int32_t));
  for (int64_t t = 0; t <= T; ++t) off[t] = f.off[(size_t)t];
  const gw::Shape sh = gw::shape(F);
  CHECK(sh.lds == (F < gw::kGlobalF) && (!sh.lds || (sh.stride % 8 == 4 && sh.stride >= F &&
                                                       (int64_t)sh.stride * gw::kRowTile <= gw::kRowTileBytes)), "shape of F");
  const int64_t blocks = (n + gw::kRowTile - 1) / gw::kRowTile;
  for (int64_t blk = 0; blk < blocks; ++blk) {
    const int64_t row0 = blk * gw::kRowTile, rows = gw::tile_rows(n, blk);
    CHECK(rows >= 1 && rows <= gw::kRowTile && row0 + rows <= n, "tile %lld", (long long)blk);
    // the tile's bytes into LDS: every byte of the range written once, inside the image
    const size_t image = sh.lds ? (size_t)sh.stride * gw::kRowTile : 1;
    uint8_t* tile = (uint8_t*)std::malloc(image);
    if (sh.lds) {
      const int bytes = (int)(rows * F);
      std::vector<int> writers(image, 0);
      const uint64_t a0 = base + (uint64_t)(row0 * F);
      const gw::Span sp = gw::span16(a0, a0 + (uint64_t)bytes);
      const uint64_t a1 = a0 + (uint64_t)bytes;
      CHECK((sp.head_end == a1 && sp.tail_begin == a1) ||
                (sp.head_end % 16 == 0 && sp.tail_begin % 16 == 0 && a0 <= sp.head_end && sp.head_end - a0 < 16 &&
                 sp.head_end < sp.tail_begin && sp.tail_begin <= a1 && a1 - sp.tail_begin < 16),
            "span of tile %lld", (long long)blk);
      const int head = (int)(sp.head_end - a0), tail = (int)(sp.tail_begin - a0);
      auto put = [&](int i) {
        const int at = gw::tile_byte(i, (int)F, sh.stride);
        CHECK(i >= 0 && i < bytes && at >= 0 && (size_t)at < image, "tile byte %d -> %d", i, at);          // W3
        if (i < 0 || i >= bytes || at < 0 || (size_t)at >= image) return;
        writers[(size_t)at] += 1;
        tile[at] = (uint8_t)bin_of(row0 + i / F, i % F);
      };
      for (int i = 0; i < head; ++i) put(i);
      for (int i = tail; i < bytes; ++i) put(i);
      for (int i = head; i < tail; i += 16)
        for (int b = 0; b < 16; ++b) put(i + b);
      int64_t written = 0;
      for (int w : writers) {
        CHECK(w <= 1, "an LDS byte written %d times", w);
        written += w;
      }
      CHECK(written == bytes, "%lld of %d bytes staged", (long long)written, bytes);
    }
    // the chunk loop, as the kernel runs it
    gw::Node* s_nodes = (gw::Node*)std::malloc(gw::kChunkNodes * sizeof(gw::Node));
    double* s_val = (double*)std::malloc(gw::kChunkNodes * sizeof(double));
    int32_t o0 = 0;
    int64_t chunks = 0, covered = 0;
    for (int64_t t0 = 0; t0 < T;) {
      const int avail = gw::window(T, t0);
      CHECK(avail >= 1 && avail <= gw::kChunkTrees && t0 + avail <= T, "window at %lld", (long long)t0);
      int32_t* win = (int32_t*)std::malloc((size_t)avail * sizeof(int32_t));      // exactly the entries that exist
      for (int i = 0; i < avail; ++i) win[i] = off[t0 + 1 + i];
      const gw::Chunk c = gw::next_chunk(win, avail, o0, (int32_t)N);
      CHECK(c.trees >= 1 && c.trees <= avail && c.nodes >= 0 && (int64_t)o0 + c.nodes <= N &&
                (c.big ? c.trees == 1 && c.nodes > gw::kChunkNodes : c.nodes <= gw::kChunkNodes),
            "chunk at tree %lld: %d trees, %d nodes", (long long)t0, c.trees, c.nodes);                     // W1, W2
      CHECK(++chunks <= T, "more chunks than trees");                                                     // W1
      if (!c.big)
        for (int32_t i = 0; i < c.nodes; ++i) {
          s_nodes[i] = f.nodes[(size_t)(o0 + i)];
          s_val[i] = value_of(o0 + i);
        }
      int32_t lo = o0;
      for (int i = 0; i < c.trees; ++i) {
        const int32_t hi = gw::clamp_off(win[i], lo, (int32_t)N), size = hi - lo;
        CHECK(lo >= o0 && hi >= lo && hi - o0 <= c.nodes, "tree %lld of the chunk", (long long)(t0 + i));
        for (int tid = 0; tid < gw::kBlock && size > 0; ++tid)
          for (int u = 0; u < gw::kRowsPerLane; ++u) {
            const int lr = gw::lane_row(tid, u);
            CHECK(lr >= 0 && lr < gw::kRowTile, "lane row");
            if (lr >= rows) continue;
            int32_t j = 0;
            for (int s = 0; s < f.steps; ++s) {
              CHECK(j >= 0 && j < size && (c.big || lo - o0 + j < gw::kChunkNodes), "node %d of %d", j, size);   // W3
              const gw::Node nd = c.big ? f.nodes[(size_t)(lo + j)] : s_nodes[lo - o0 + j];
              const int64_t ft = gw::bin_feature(nd, size, F);
              CHECK(ft >= 0 && ft < F, "feature %lld", (long long)ft);                                   // W3
              const int bin = sh.lds ? tile[(int64_t)lr * sh.stride + ft] : bin_of(row0 + lr, ft);
              const int32_t nx = gw::step(nd, size, F, bin);
              CHECK(nx < size, "next node %d of %d", nx, size);
              j = nx >= 0 ? nx : j;
            }
            got[(size_t)(row0 + lr)] += c.big ? value_of(lo + j) : s_val[lo - o0 + j];
            got_leaf[(size_t)((row0 + lr) * T + t0 + i)] = j;
          }
        if (size == 0)
          for (int64_t r = 0; r < rows; ++r) got_leaf[(size_t)((row0 + r) * T + t0 + i)] = -1;
        lo = hi;
      }
      CHECK(lo - o0 == c.nodes, "the chunk's trees hold its nodes");
      covered += c.trees;
      o0 += c.nodes;
      t0 += c.trees;
      std::free(win);
    }
    CHECK(covered == T, "%lld of %lld trees covered", (long long)covered, (long long)T);                   // W2
    std::free(s_val);
    std::free(s_nodes);
    std::free(tile);
  }
  CHECK(std::memcmp(got.data(), want.data(), (size_t)n * sizeof(double)) == 0, "pred, F = %lld", (long long)F);   // W4
  CHECK(got_leaf == want_leaf, "leaf, F = %lld", (long long)F);
  std::free(off);
}

int main() {
  const int64_t Fs[] = {1, 3, 37, gw::kGlobalF};
  size_t count = 0;
  for (int64_t F : Fs) {
    std::vector<Forest> fs;
    fs.push_back(Forest{"T = 0", {}, {0}, 6});
    {
      Forest f{"one leaf, steps = 0", {}, {0}, 0};
      add_tree(f, 0, F);
      fs.push_back(f);
    }
    {
      Forest f{"depth-6 trees across two chunks", {}, {0}, 6};       // 127 nodes a tree: 4 fit, the 5th crosses
      for (int t = 0; t < 5; ++t) add_tree(f, 6, F);
      fs.push_back(f);
    }
    {
      Forest f{"one big tree, then small ones", {}, {0}, gw::kMaxSteps};
      add_chain(f, gw::kChunkNodes + 1);                            // a path far past kMaxSteps: the walk stops at steps
      for (int t = 0; t < 3; ++t) add_tree(f, 2, F);
      fs.push_back(f);
    }
    {
      Forest f{"more stumps than a window", {}, {0}, 1};
      for (int t = 0; t < gw::kChunkTrees + 9; ++t) add_tree(f, 1, F);
      fs.push_back(f);
    }
    {
      Forest f{"hostile nodes", {}, {0}, 9};
      f.nodes = {{0, 100, 0, 0},                                                   // tree 0: a self-loop
                 {0, -2147483647 - 1, 1, 1}, {0, 2147483647, 0, 0}, {-1, 0, -1, -1},   // tree 1: a two-node cycle
                 {0, 50, 1, 2}, {0, 0, 5, 0}, {0, 0, 0, -4},                       // tree 2: children outside the tree
                 {(int32_t)F, 7, 1, 1}, {0, 7, 0, 0}};                             // tree 3: a feature >= F
      f.off = {0, 1, 4, 7, 9};
      fs.push_back(f);
    }
    {
      Forest f{"hostile tree_off", {}, {0}, 3};
      for (int t = 0; t < 6; ++t) add_tree(f, 2, F);   // 42 nodes; the table below disagrees with them
      f.off = {99, -5, 7, 3, 2147483647, 12, -2147483647 - 1, 42};
      fs.push_back(f);
    }
    for (const Forest& f : fs)
      for (int64_t n : {(int64_t)1, (int64_t)gw::kRowTile + 17})
        for (uint64_t base : {(uint64_t)4096, (uint64_t)4099}) {
          run(f, n, F, base);
          ++count;
        }
  }
  {
    const Forest& f = Forest{"tiny tiles", {}, {0}, 0};
    for (int64_t n = 1; n < 40; ++n) run(f, n, 3, 4093);                        // ranges that hold no aligned 16 bytes
  }
  return map_test::report("OK %zu walks\n", count);
}
