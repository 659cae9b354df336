// tests/native/ddpg_vars_tool.cpp -- the DDPG handle's variable table, its initial-value rule and the re-lay of an arena
// (ga3c_amd/csrc/ga3c_ddpg_vars.hpp) on their own, held to numpy without a GPU (tests/test_ddpg_vars_cpu.py).
// <options>: eight integers, S A atoms head twin pop soft critic_adam.
//   ddpg_vars_tool table <options>       one line per variable, tab separated: name, offset, count, shape (a,b), trainable,
//                                        checkpoint members (member=arena,...), the target copy's name; then "n <arena size>"
//   ddpg_vars_tool relay <options of the old table> <options of the new one> <log_alpha> <in> <out>
//                                        <in>: the five old arenas, f32; <out>: the five arenas re-laid, f32
//   ddpg_vars_tool fresh <options> <log_alpha> <out>    the five arenas re-laid from an empty table: a new handle's
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../ga3c_amd/csrc/ga3c_ddpg_vars.hpp"

using namespace ga3c_dd;

static Options options(char** a) {
  Options o;
  o.S = atoi(a[0]); o.A = atoi(a[1]); o.atoms = atoi(a[2]); o.head = atoi(a[3]);
  o.twin = atoi(a[4]) != 0; o.pop = atoi(a[5]) != 0; o.soft = atoi(a[6]) != 0; o.critic_adam = atoi(a[7]) != 0;
  return o;
}

int main(int argc, char** argv) {
  if (argc == 10 && !strcmp(argv[1], "table")) {
    const Table t = make_table(options(argv + 2));
    for (size_t i = 0; i < t.vars.size(); ++i) {
      const ga3c_ckpt::Var& v = t.vars[i];
      printf("%s\t%lld\t%lld\t", v.name.c_str(), (long long)v.off, (long long)v.count);
      for (int d = 0; d < v.ndim; ++d) printf("%s%lld", d ? "," : "", (long long)v.shape[d]);
      printf("\t%d\t", trainable(v) ? 1 : 0);
      for (size_t k = 0; k < v.ckpt.size(); ++k) printf("%s%s=%d", k ? "," : "", v.ckpt[k].first.c_str(), v.ckpt[k].second);
      printf("\t%s\n", t.tnames[i].c_str());
    }
    printf("n %lld\n", (long long)t.n);
    return 0;
  }
  const bool fresh = argc == 12 && !strcmp(argv[1], "fresh");
  if (!fresh && !(argc == 21 && !strcmp(argv[1], "relay"))) return 2;
  const Table from = fresh ? Table{} : make_table(options(argv + 2)), to = make_table(options(argv + (fresh ? 2 : 10)));
  const float log_alpha = (float)atof(argv[fresh ? 10 : 18]);
  FILE* in = fresh ? nullptr : fopen(argv[19], "rb");
  FILE* out = fopen(argv[argc - 1], "wb");
  if ((!fresh && !in) || !out) return 2;
  std::vector<float> old((size_t)from.n);
  for (int a = 0; a < 5; ++a) {
    if (in && fread(old.data(), sizeof(float), old.size(), in) != old.size()) return 2;
    const std::vector<float> laid = relay(from, old, to, a, log_alpha);
    if (laid.size() != (size_t)to.n || fwrite(laid.data(), sizeof(float), laid.size(), out) != laid.size()) return 2;
  }
  if (in) fclose(in);
  return fclose(out) ? 2 : 0;
}
