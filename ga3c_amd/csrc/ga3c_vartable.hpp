// ga3c_vartable.hpp -- the variable table every network handle keeps (ga3c_engine.hip, ga3c_mlp.hip, ga3c_dmlp.hip,
// ga3c_ddpg.hip) and the one path between that table and a checkpoint (ga3c_checkpoint.hpp): which members a variable is kept
// under, how the host copies of the arenas become members and how members become arenas again.  Host code only: nothing
// here knows a device, a lock or a handle.  The caller reads its arenas to the host before pack_members and writes them back
// after unpack_members.
#pragma once
#include <algorithm>
#include <utility>

#include "ga3c_checkpoint.hpp"

namespace ga3c_ckpt {

struct Var {                      // one variable: its name (no ":0"), its first arena element, its shape, and the
  std::string name;               // (member name, arena) pairs a checkpoint keeps it under
  int64_t off, count;
  int32_t ndim;
  int64_t shape[4];
  std::vector<std::pair<std::string, int>> ckpt;
};

typedef std::vector<std::vector<float>> Arenas;     // by arena number; an arena no member names may stay empty

// index of the variable called `name` (with or without ":0"), or -1
inline int find_var(const std::vector<Var>& vars, const char* name) {
  if (!name) return -1;
  std::string s(name);
  if (s.size() > 2 && s.compare(s.size() - 2, 2, ":0") == 0) s.resize(s.size() - 2);
  for (size_t i = 0; i < vars.size(); ++i)
    if (s == vars[i].name) return (int)i;
  return -1;
}

// One RMSProp optimizer (tf.train.Saver names, NetworkVP.py:62-64): the variable in arena 0, its `ms` slot in 1, `mom` in 2.
inline void single_members(Var* var) {
  var->ckpt = {{var->name + ":0", 0}, {var->name + "/RMSProp:0", 1}, {var->name + "/RMSProp_1:0", 2}};
}

// DUAL_RMSPROP, one optimizer per cost: `value` / `policy` say whether the optimizer of cost_v / of cost_p has slots for the
// variable (the trunk: both; a head: its own).  Derived, not observed (no TensorFlow here; unverified against a TF run): both
// branches build the value optimizer first (NetworkVP_discrate.py:109-112 and :126), TF-1's RMSPropOptimizer._create_slots
// makes the `rms` slot, then the `momentum` slot of each variable, both named after the optimizer ("RMSProp"), and uniquifies
// a repeated name with _1, _2, ...  An optimizer has no slot for a variable its cost has no gradient for.  So the trunk
// carries the value optimizer's slots as RMSProp / RMSProp_1 and the policy optimizer's as RMSProp_2 / RMSProp_3, and a head
// its one optimizer's as RMSProp / RMSProp_1 -- single_members' rule applied twice.  The value optimizer's `ms` / `mom` are
// arenas 4 / 5, the policy optimizer's 1 / 2.
inline void dual_members(Var* var, bool value, bool policy) {
  var->ckpt = {{var->name + ":0", 0}};
  if (value) {
    var->ckpt.emplace_back(var->name + "/RMSProp:0", 4);
    var->ckpt.emplace_back(var->name + "/RMSProp_1:0", 5);
  }
  if (policy) {
    var->ckpt.emplace_back(var->name + (value ? "/RMSProp_2:0" : "/RMSProp:0"), 1);
    var->ckpt.emplace_back(var->name + (value ? "/RMSProp_3:0" : "/RMSProp_1:0"), 2);
  }
}

// What a checkpoint holds: "step", then the members of every variable in table order.
inline std::vector<Member> pack_members(const std::vector<Var>& vars, int64_t step, const Arenas& arena) {
  std::vector<Member> members(1);
  members[0].name = "step";
  members[0].descr = "<i8";
  members[0].bytes.assign(reinterpret_cast<const uint8_t*>(&step), reinterpret_cast<const uint8_t*>(&step) + 8);
  for (const Var& var : vars)
    for (const auto& km : var.ckpt) {
      Member mb;
      mb.name = km.first;
      mb.descr = "<f4";
      mb.shape.assign(var.shape, var.shape + var.ndim);
      const uint8_t* src = reinterpret_cast<const uint8_t*>(arena[km.second].data() + var.off);
      mb.bytes.assign(src, src + (size_t)var.count * sizeof(float));
      members.push_back(std::move(mb));
    }
  return members;
}

inline bool checkpoint_step(const std::string& path, const std::map<std::string, Member>& members, int64_t* step,
                            std::string* err) {
  auto st = members.find("step");
  if (st == members.end() || st->second.descr != "<i8" || st->second.bytes.size() != 8) {
    *err = path + " holds no int64 step";
    return false;
  }
  memcpy(step, st->second.bytes.data(), 8);
  return true;
}

// `members`: the file `path`, read already; `kind`: what the network calls itself.  Every member the table names must be
// there as <f4 of the variable's shape, and the step as int64: a file of another network kind lacks this one's first
// variable.  All of that is checked before the first element is copied; false + *err leaves *arena and *step as they were.
// An arena element that no member names keeps the value the caller gave it.
inline bool unpack_members(const std::string& path, const char* kind, const std::vector<Var>& vars,
                           const std::map<std::string, Member>& members, Arenas* arena, int64_t* step, std::string* err) {
  for (const Var& var : vars)
    for (const auto& km : var.ckpt) {
      auto it = members.find(km.first);
      if (it == members.end()) {
        *err = path + " holds no " + km.first + ": not a checkpoint of this " + kind;
        return false;
      }
      const Member& mb = it->second;
      const bool shape_ok = mb.shape.size() == (size_t)var.ndim && std::equal(mb.shape.begin(), mb.shape.end(), var.shape);
      if (mb.descr != "<f4" || !shape_ok || mb.bytes.size() != (size_t)var.count * sizeof(float)) {
        *err = path + ": " + km.first + " is not <f4 of this network's shape (" + std::to_string((long long)var.count) + " elements)";
        return false;
      }
    }
  if (!checkpoint_step(path, members, step, err)) return false;
  for (const Var& var : vars)
    for (const auto& km : var.ckpt) {
      const Member& mb = members.find(km.first)->second;
      memcpy((*arena)[km.second].data() + var.off, mb.bytes.data(), mb.bytes.size());
    }
  return true;
}

}  // namespace ga3c_ckpt
