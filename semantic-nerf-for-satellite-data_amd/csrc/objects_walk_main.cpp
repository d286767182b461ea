// The union-find walk of snerf_objects_link (objects_walk.h) on the host, before it runs on a GPU: the merge and the flatten of
// csrc/objects.hip over std::atomic<int>, 16 threads, shuffled cell orders, under ThreadSanitizer (`make objects-walk`), each result
// compared with a sequential flood fill written here; the guard counter must stay 0.  No HIP in this program; CPU machines only.
#include "objects_walk.h"

#include <algorithm>
#include <atomic>
#include <cstdio>
#include <numeric>
#include <random>
#include <string>
#include <thread>
#include <vector>

namespace {

constexpr int THREADS = 16;
constexpr int ORDERS = 3;              // shuffled cell orders per raster and connectivity

struct HostParents {
  std::atomic<int>* parent;
  int load(int c) { return parent[c].load(std::memory_order_relaxed); }
  int fetch_min(int c, int v) {
    int old = parent[c].load(std::memory_order_relaxed);
    while (old > v && !parent[c].compare_exchange_weak(old, v, std::memory_order_relaxed)) {}
    return old;
  }
};

struct Raster {
  std::string name;
  int h, w;
  std::vector<unsigned char> label;
};

bool member(unsigned char l) { return l == 3 || l == 4; }

// the labelling the header describes, sequentially: a flood fill from every unvisited member cell in raster order, whose start is
// therefore the smallest index of its component
std::vector<int> flood(const Raster& r, bool eight) {
  std::vector<int> parent(r.h * r.w, -1), stack;
  std::vector<char> seen(r.h * r.w, 0);
  for (int c = 0; c < r.h * r.w; ++c) {
    if (!member(r.label[c]) || seen[c]) continue;
    seen[c] = 1;
    stack.push_back(c);
    while (!stack.empty()) {
      const int a = stack.back();
      stack.pop_back();
      parent[a] = c;
      const int j = a / r.w, i = a % r.w;
      for (int dj = -1; dj <= 1; ++dj)
        for (int di = -1; di <= 1; ++di) {
          if ((!dj && !di) || (!eight && dj && di)) continue;
          const int nj = j + dj, ni = i + di;
          if (nj < 0 || nj >= r.h || ni < 0 || ni >= r.w) continue;
          const int n = nj * r.w + ni;
          if (seen[n] || r.label[n] != r.label[a]) continue;
          seen[n] = 1;
          stack.push_back(n);
        }
    }
  }
  return parent;
}

// the merge step of one cell, as link_merge_kernel (link_kernels.h) makes it
int merge_cell(HostParents& m, const Raster& r, bool eight, int c) {
  const unsigned char l = r.label[c];
  if (!member(l)) return 0;
  const int j = c / r.w, i = c % r.w;
  int trips = 0;
  if (i > 0 && r.label[c - 1] == l) trips += snerf::walk_unite(m, c, c - 1);
  if (j > 0) {
    const int n = c - r.w;
    if (r.label[n] == l) trips += snerf::walk_unite(m, c, n);
    if (eight && i > 0 && r.label[n - 1] == l) trips += snerf::walk_unite(m, c, n - 1);
    if (eight && i + 1 < r.w && r.label[n + 1] == l) trips += snerf::walk_unite(m, c, n + 1);
  }
  return trips;
}

template <typename F>
void in_threads(int cells, F&& body) {
  std::vector<std::thread> pool;
  for (int t = 0; t < THREADS; ++t)
    pool.emplace_back([&, t] {
      for (int k = t; k < cells; k += THREADS) body(k);      // interleaved: neighbours in the order go to different threads
    });
  for (auto& th : pool) th.join();
}

int run(const Raster& r, bool eight, unsigned seed, long long* unions) {
  const int cells = r.h * r.w;
  std::vector<std::atomic<int>> parent(cells);
  for (int c = 0; c < cells; ++c) parent[c].store(member(r.label[c]) ? c : -1, std::memory_order_relaxed);
  std::vector<int> order(cells);
  std::iota(order.begin(), order.end(), 0);
  std::mt19937 rng(seed);
  if (seed) std::shuffle(order.begin(), order.end(), rng);  // seed 0: the raster order, as the kernel's threads are numbered
  HostParents m = {parent.data()};
  std::atomic<long long> trips(0);
  in_threads(cells, [&](int k) { if (int t = merge_cell(m, r, eight, order[k])) trips += t; });
  in_threads(cells, [&](int k) {
    const int c = order[k];
    if (m.load(c) < 0) return;
    const int root = snerf::walk_find(m, c);
    if (root < 0) { trips += 1; return; }
    parent[c].store(root, std::memory_order_relaxed);
  });
  const std::vector<int> want = flood(r, eight);
  int wrong = 0;
  long long members = 0;
  for (int c = 0; c < cells; ++c) {
    wrong += parent[c].load(std::memory_order_relaxed) != want[c];
    members += want[c] >= 0;
  }
  *unions += members;
  if (wrong || trips.load())
    printf("%-28s connectivity %d order %u: %d wrong words, %lld guard trips   <-- UNEXPECTED\n", r.name.c_str(), eight ? 8 : 4, seed, wrong,
           trips.load());
  return (wrong ? 1 : 0) + (trips.load() ? 1 : 0);
}

Raster filled(const char* name, int h, int w, unsigned char v) { return {name, h, w, std::vector<unsigned char>((size_t)h * w, v)}; }

std::vector<Raster> rasters() {
  std::vector<Raster> out;
  const unsigned char drawn[4] = {0, 3, 4, 255};
  const int shapes[][2] = {{1, 1}, {1, 130}, {130, 1}, {7, 65}, {33, 64}, {70, 129}};
  std::mt19937 rng(7);
  for (auto& s : shapes) {
    Raster r = filled("random", s[0], s[1], 0);
    r.name += " " + std::to_string(s[0]) + "x" + std::to_string(s[1]);
    for (auto& l : r.label) l = drawn[rng() & 3];
    out.push_back(r);
  }
  {  // serpentine: full rows at even j, joined alternately at the east and the west end: one component, chains ~1,100 long
    Raster r = filled("serpentine 33x67", 33, 67, 0);
    for (int j = 0; j < 33; ++j)
      for (int i = 0; i < 67; ++i)
        if (j % 2 == 0 || i == ((j / 2) % 2 == 0 ? 66 : 0)) r.label[j * 67 + i] = 3;
    out.push_back(r);
  }
  {  // square spiral: walls on every second ring, each ring opened into the next
    Raster r = filled("spiral 65x65", 65, 65, 0);
    const int n = 65;
    int j = 0, i = 0, dj = 0, di = 1, turns = 0;
    std::vector<char> on(n * n, 0);
    on[0] = 1;
    auto is_on = [&](int jj, int ii) { return jj >= 0 && jj < n && ii >= 0 && ii < n && on[jj * n + ii]; };
    while (turns < 2) {      // a step ahead is free while it stays inside, off the path and one cell clear of it; else turn right
      const int nj = j + dj, ni = i + di;
      if (nj >= 0 && nj < n && ni >= 0 && ni < n && !on[nj * n + ni] && !is_on(nj + dj, ni + di)) {
        j = nj, i = ni, on[j * n + i] = 1, turns = 0;
      } else {
        const int t = dj;
        dj = di, di = -t, ++turns;
      }
    }
    for (int c = 0; c < n * n; ++c) r.label[c] = on[c] ? 3 : 0;
    out.push_back(r);
  }
  {
    Raster r = filled("checkerboard 16x70", 16, 70, 0);
    for (int j = 0; j < 16; ++j)
      for (int i = 0; i < 70; ++i) r.label[j * 70 + i] = (i + j) % 2 ? 0 : 3;
    out.push_back(r);
  }
  out.push_back(filled("one class 64x256", 64, 256, 3));
  {  // a comb whose teeth meet only in the last row
    Raster r = filled("comb 40x129", 40, 129, 0);
    for (int j = 0; j < 40; ++j)
      for (int i = 0; i < 129; ++i)
        if (i % 2 == 0 || j == 39) r.label[j * 129 + i] = 4;
    out.push_back(r);
  }
  {  // two participating classes in alternating columns: never merged
    Raster r = filled("alternating columns 20x66", 20, 66, 0);
    for (int j = 0; j < 20; ++j)
      for (int i = 0; i < 66; ++i) r.label[j * 66 + i] = i % 2 ? 4 : 3;
    out.push_back(r);
  }
  out.push_back(filled("no member 9x70", 9, 70, 255));
  return out;
}

}  // namespace

int main() {
  int failures = 0, runs = 0;
  long long unions = 0;
  for (const Raster& r : rasters())
    for (int eight = 0; eight < 2; ++eight)
      for (unsigned seed = 0; seed <= ORDERS; ++seed, ++runs) failures += run(r, eight != 0, seed, &unions);
  printf("objects walk: %d runs (%d threads, raster order + %d shuffled orders, connectivity 4 and 8), %lld member cells, %s\n", runs,
         THREADS, ORDERS, unions, failures ? "FAILED" : "ok");
  return failures ? 1 : 0;
}
