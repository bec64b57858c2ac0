// The container Open3D's VoxelDownSample iterates: a libstdc++ std::unordered_map keyed on the voxel index triple with
// utility::hash_eigen, filled in first-occurrence order.  Reads int32 triples [n,3] from argv[1], writes int64 [m] to argv[2]:
// the insertion rank of every distinct triple in iteration order.  Built with g++ by tests/test_voxel_down_sample_cpu.py.
#include <array>
#include <cstdint>
#include <cstdio>
#include <unordered_map>
#include <vector>

struct HashEigen {   // boost hash_combine over std::hash<int>, as utility::hash_eigen<Eigen::Vector3i>
  std::size_t operator()(const std::array<int, 3>& k) const {
    std::size_t seed = 0;
    for (int e : k) seed ^= std::hash<int>()(e) + 0x9e3779b9 + (seed << 6) + (seed >> 2);
    return seed;
  }
};

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 3;
  std::vector<std::array<int, 3>> idx;
  std::array<int, 3> k;
  while (std::fread(k.data(), sizeof(int), 3, f) == 3) idx.push_back(k);
  std::fclose(f);
  std::unordered_map<std::array<int, 3>, int64_t, HashEigen> map;
  for (const auto& t : idx) map.emplace(t, static_cast<int64_t>(map.size()));   // no-op for a voxel already present
  std::vector<int64_t> order;
  for (const auto& kv : map) order.push_back(kv.second);
  FILE* g = std::fopen(argv[2], "wb");
  if (!g) return 4;
  std::fwrite(order.data(), sizeof(int64_t), order.size(), g);
  std::fclose(g);
  return 0;
}
