// ga3c_ddpg_vars.hpp -- the variables of a DDPG handle (ga3c_ddpg.hip): their names and arena layout, the one builder of the
// variable table for whatever options the handle carries, the one rule for a variable's initial value, and the re-lay of an
// arena image from one table to another.  DESIGN.md 8v.  Host code only, plain C++17: nothing here knows a device, a lock or a
// handle (tests/native/ddpg_vars_tool.cpp holds it to numpy without a GPU).
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "ga3c_vartable.hpp"

namespace ga3c_dd {

constexpr int H1 = 400;
constexpr int H2 = 300;

// Variables, arena order: the actor's trainable ones, the critic's, then the moving statistics.
enum {
  A_W1, A_B1, A_BE1, A_GA1, A_W2, A_B2, A_BE2, A_GA2, A_WO, A_BO,
  C_W1, C_B1, C_BE1, C_GA1, C_W2, C_B2DEAD, C_WN, C_BN, C_WO, C_BO,
  A_MM1, A_MV1, A_MM2, A_MV2, C_MM1, C_MV1, NVARS
};
constexpr int NTRAIN = 20;             // variables 0..19 are trainable
constexpr int NACTOR = 10;             // ... 0..9 the actor's

const char* const VAR_NAMES[NVARS] = {
    "actor_fc1/W", "actor_fc1/b", "actor_norm1/beta", "actor_norm1/gamma", "actor_fc2/W", "actor_fc2/b", "actor_norm2/beta",
    "actor_norm2/gamma", "actor_output/W", "actor_output/b",
    "critic_fc1/W", "critic_fc1/b", "critic_norm1/beta", "critic_norm1/gamma", "critic_fc2/W", "critic_fc2/b", "critic_norm2/W",
    "critic_norm2/b", "critic_output/W", "critic_output/b",
    "actor_norm1/moving_mean", "actor_norm1/moving_variance", "actor_norm2/moving_mean", "actor_norm2/moving_variance",
    "critic_norm1/moving_mean", "critic_norm1/moving_variance"};

// ... and the twin's (ga3c_ddpg_twin_create): critic 2's, variables 26..37 of such a handle
const char* const TWIN_VAR_NAMES[12] = {
    "critic2_fc1/W", "critic2_fc1/b", "critic2_norm1/beta", "critic2_norm1/gamma", "critic2_fc2/W", "critic2_fc2/b", "critic2_norm2/W",
    "critic2_norm2/b", "critic2_output/W", "critic2_output/b", "critic2_norm1/moving_mean", "critic2_norm1/moving_variance"};

// ... PopArt's statistics (ga3c_ddpg_popart_create) and the soft actor-critic's temperature (ga3c_ddpg_soft_create), f32 (1,)
const char* const POP_VAR_NAMES[2] = {"critic_popart/mu", "critic_popart/nu"};
const char* const SOFT_VAR_NAME = "actor_soft/log_alpha";

struct Layout {
  int S, A;
  int rows[NVARS], cols[NVARS];    // a vector has rows = 0
  int64_t off[NVARS + 1];
};

// N: the outputs of the critic's head, 1 or the atoms of a distributional critic
// head: the columns of the actor's head, A, or 2 A for the Gaussian head of a soft handle (0: A)
inline Layout make_layout(int S, int A, int N = 1, int head = 0) {
  Layout L;
  L.S = S;
  L.A = A;
  const int HD = head ? head : A;
  const int r[NVARS] = {S, 0, 0, 0, H1, 0, 0, 0, H2, 0, S, 0, 0, 0, H1, 0, A, 0, H2, 0, 0, 0, 0, 0, 0, 0};
  const int c[NVARS] = {H1, H1, H1, H1, H2, H2, H2, H2, HD, HD, H1, H1, H1, H1, H2, H2, H2, H2, N, N, H1, H1, H2, H2, H1, H1};
  int64_t o = 0;
  for (int v = 0; v < NVARS; ++v) {
    L.rows[v] = r[v];
    L.cols[v] = c[v];
    L.off[v] = o;
    o += (int64_t)(r[v] ? r[v] : 1) * c[v];
  }
  L.off[NVARS] = o;
  return L;
}

// The twin's twelve variables lie behind the 26, in the critic's order: its ten trainable ones, then its moving statistics.
constexpr int NTWIN = 12;
constexpr int NCRITIC = NTRAIN - NACTOR;

// L with the critic's entries naming critic 2's variables: off[NACTOR .. NTRAIN] its trainable ones and their end, off[C_MM1],
// off[C_MV1] its statistics.  The actor's statistics have no meaning in the view; no critic code reads them.
inline Layout twin_view(const Layout& L) {
  Layout V = L;
  const int64_t shift = L.off[NVARS] - L.off[NACTOR];
  for (int v = NACTOR; v <= NTRAIN; ++v) V.off[v] = L.off[v] + shift;
  for (int v = NTRAIN + 1; v < C_MM1; ++v) V.off[v] = V.off[NTRAIN];
  V.off[C_MM1] = V.off[NTRAIN];
  V.off[C_MV1] = V.off[C_MM1] + H1;
  V.off[NVARS] = V.off[C_MV1] + H1;
  return V;
}

// tflearn's name of the target copy: the layer's scope is made a second time, "actor_fc1" -> "actor_fc1_1" (the one place).
inline std::string target_name(const std::string& s) {
  const size_t slash = s.find('/');
  return s.substr(0, slash) + "_1" + s.substr(slash);
}

// What fixes a handle's variables.
struct Options {
  int S = 0, A = 0;
  int atoms = 1;               // the critic head's outputs: 1, or the atoms of a distributional critic
  int head = 0;                // the actor head's columns: A (0 says so too), or 2 A on a soft handle
  bool twin = false;           // critic 2's twelve
  bool pop = false;            // PopArt's mu, nu
  bool soft = false;           // log_alpha
  bool critic_adam = false;    // GA3C_DDPG_CRITIC_ADAM: which names the critics' optimizer slots go by
};

struct Table {
  Layout L{};                            // the 26's
  Layout view{};                         // twin_view(L): critic 2's, of a table with `twin`
  std::vector<ga3c_ckpt::Var> vars;      // arena order, contiguous from 0 to n
  std::vector<std::string> tnames;       // the target copies' names, by variable
  int64_t n = 0;                         // arena size
};

// The whole table: the 26, then critic 2's twelve read through the twin's view, then PopArt's two, then log_alpha.  Value and
// target copy of every variable are checkpoint members; a trainable one also has the two slots of its optimizer, under Adam's
// names (the actor's, log_alpha's, and the critics' under `critic_adam`) or RMSProp's.
inline Table make_table(const Options& o) {
  Table t;
  t.L = make_layout(o.S, o.A, o.atoms, o.head);
  t.view = twin_view(t.L);
  auto add = [&](std::string name, int64_t off, int rows, int cols, const char* slots) {
    ga3c_ckpt::Var var{name, off, (int64_t)(rows ? rows : 1) * cols, 1, {cols, 0}, {}};
    if (rows) {                                    // a matrix [rows, cols]; a vector has rows = 0
      var.ndim = 2;
      var.shape[0] = rows;
      var.shape[1] = cols;
    }
    var.ckpt = {{name + ":0", 0}, {target_name(name) + ":0", 1}};
    if (slots) {
      var.ckpt.emplace_back(name + "/" + slots + ":0", 2);
      var.ckpt.emplace_back(name + "/" + slots + "_1:0", 3);
    }
    t.n = off + var.count;
    t.vars.push_back(std::move(var));
  };
  // variable i of layout `L` (a view: the critic's entries only)
  auto of_layout = [&](const Layout& L, int i, const char* name) {
    add(name, L.off[i], L.rows[i], L.cols[i], i >= NTRAIN ? nullptr : i < NACTOR || o.critic_adam ? "Adam" : "RMSProp");
  };
  for (int i = 0; i < NVARS; ++i) of_layout(t.L, i, VAR_NAMES[i]);
  if (o.twin) {
    for (int i = 0; i < NCRITIC; ++i) of_layout(t.view, NACTOR + i, TWIN_VAR_NAMES[i]);
    of_layout(t.view, C_MM1, TWIN_VAR_NAMES[NCRITIC]);
    of_layout(t.view, C_MV1, TWIN_VAR_NAMES[NCRITIC + 1]);
  }
  if (o.pop)                                       // not trainable: no slots
    for (const char* name : POP_VAR_NAMES) add(name, t.n, 0, 1, nullptr);
  if (o.soft) add(SOFT_VAR_NAME, t.n, 0, 1, "Adam");
  for (const ga3c_ckpt::Var& var : t.vars) t.tnames.push_back(target_name(var.name));
  return t;
}

// A variable is trainable iff it has optimizer-slot members.
inline bool trainable(const ga3c_ckpt::Var& var) { return var.ckpt.size() > 2; }

// The value a variable starts from in arena `arena` (value, target, slot a, slot b, gradient), the one statement of it:
//   a moving variance and PopArt's nu    1 in the value and the target arena
//   log_alpha                            `log_alpha` in those two
//   a critic's trainable variable        1 in slot a, TF-1 RMSProp's ms, unless the critic is on Adam (only a critic's variable
//                                        has RMSProp's slot members; the dead critic_fc2/b is one of them)
//   everything else                      0
inline float initial_value(const ga3c_ckpt::Var& var, int arena, float log_alpha) {
  static const std::string mv = "/moving_variance", rms = "/RMSProp:0";
  auto ends = [](const std::string& s, const std::string& tail) {
    return s.size() >= tail.size() && s.compare(s.size() - tail.size(), tail.size(), tail) == 0;
  };
  if (arena <= 1) {
    if (ends(var.name, mv) || var.name == POP_VAR_NAMES[1]) return 1.f;
    return var.name == SOFT_VAR_NAME ? log_alpha : 0.f;
  }
  return arena == 2 && trainable(var) && ends(var.ckpt[2].first, rms) ? 1.f : 0.f;
}

// The image of arena `arena` under table `to`, from its image `old` under table `from`: a variable keeps its elements where
// `from` has a variable of the same name and the same shape, and starts from initial_value otherwise.  An empty `from` gives the
// arena of a new handle.
inline std::vector<float> relay(const Table& from, const std::vector<float>& old, const Table& to, int arena, float log_alpha) {
  std::vector<float> laid((size_t)to.n);
  for (const ga3c_ckpt::Var& var : to.vars) {
    const int j = ga3c_ckpt::find_var(from.vars, var.name.c_str());
    const ga3c_ckpt::Var* was = j < 0 ? nullptr : &from.vars[(size_t)j];
    if (was && was->ndim == var.ndim && std::equal(var.shape, var.shape + var.ndim, was->shape))
      std::copy(old.begin() + was->off, old.begin() + was->off + was->count, laid.begin() + var.off);
    else
      std::fill(laid.begin() + var.off, laid.begin() + var.off + var.count, initial_value(var, arena, log_alpha));
  }
  return laid;
}

}  // namespace ga3c_dd
