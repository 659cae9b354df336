// tests/native/vartable_tool.cpp -- the variable table and its checkpoint path (ga3c_amd/csrc/ga3c_vartable.hpp) on their own,
// held to numpy without a GPU (tests/test_vartable_cpu.py).  The table is a small two-optimizer network: two trunk layers, a
// value head and a policy head, members by the shared DUAL_RMSPROP rule.  Seven arenas of the table's 43 elements.
//   vartable_tool write <out.npz> <step>   arena w, element i = i + w / 8; pack_members + write_npz
//   vartable_tool read <in.npz> <dump>     arenas and step filled with -1, then read_npz + unpack_members; <dump> gets the
//                                          step (int64) and the seven arenas (f32) as they are afterwards, refused or not;
//                                          exit 1 and the reason on stderr when the file is refused
//   vartable_tool find <name>              prints find_var's index
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../ga3c_amd/csrc/ga3c_checkpoint.hpp"
#include "../../ga3c_amd/csrc/ga3c_vartable.hpp"

using namespace ga3c_ckpt;

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  std::vector<Var> vars = {{"fc1/w", 0, 12, 2, {3, 4}, {}},    {"fc1/b", 12, 4, 1, {4}, {}},    {"fc2/w", 16, 12, 2, {4, 3}, {}},
                           {"fc2/b", 28, 3, 1, {3}, {}},       {"head_v/w", 31, 3, 2, {3, 1}, {}}, {"head_v/b", 34, 1, 1, {1}, {}},
                           {"head_p/w", 35, 6, 2, {3, 2}, {}}, {"head_p/b", 41, 2, 1, {2}, {}}};
  const size_t n = 43;
  for (size_t i = 0; i < vars.size(); ++i) dual_members(&vars[i], i < 6, i < 4 || i >= 6);
  std::string err;
  if (!strcmp(argv[1], "find")) {
    printf("%d\n", find_var(vars, argv[2]));
    return 0;
  }
  if (argc < 4) return 2;
  Arenas arena(7, std::vector<float>(n));
  if (!strcmp(argv[1], "write")) {
    for (int w = 0; w < 7; ++w)
      for (size_t i = 0; i < n; ++i) arena[w][i] = (float)i + (float)w / 8;
    if (!write_npz(argv[2], pack_members(vars, atoll(argv[3]), arena), &err)) { fprintf(stderr, "%s\n", err.c_str()); return 1; }
    return 0;
  }
  for (auto& a : arena) a.assign(n, -1.0f);
  int64_t step = -1;
  std::map<std::string, Member> members;
  const bool ok = read_npz(argv[2], &members, &err) && unpack_members(argv[2], "test network", vars, members, &arena, &step, &err);
  FILE* f = fopen(argv[3], "wb");
  if (!f) return 2;
  fwrite(&step, 8, 1, f);
  for (auto& a : arena) fwrite(a.data(), sizeof(float), n, f);
  fclose(f);
  if (!ok) fprintf(stderr, "%s\n", err.c_str());
  return ok ? 0 : 1;
}
