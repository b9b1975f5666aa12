// moog_fops.h -- the flattened force list of a program: ONE definition, for the host (the list the engine copies to device
// memory for the generic step kernels), for a program-specialised build (the list as a constant of the translation unit:
// moog_device.h, EFOP / ENFOPS) and for plain C++ (tests/test_step_spec_fops.py compiles it with the host compiler).
// No HIP, no allocation in the constexpr path.
#pragma once
#include <stdint.h>
#include <vector>   // (moog_flatten_forces only: the host's wrapper at the bottom)

#include "../../include/moog_engine.h"

// One entry of the flattened force list: a (force, layer a, layer b) combination of physics.py:96-108 with everything its
// loop header needs in 64 contiguous bytes (one scalar load), built once per engine on the host (moog_flatten_forces).
// The nested loops over program.forces read ~10 dependent scalars per combination -- force kind, list
// lengths, layer ids, slot ranges, the Collision parameters -- ten times per env-step: 6 % of the contact-heavy envs'
// cycles and 12 % of the typical env's sat in those headers (profiles/r04_step_sections.txt).
struct FOp {
  int32_t fi, kind;          // index into program.forces (the rarely used kinds still read their record), MOOG_FORCE_*
  int32_t a0, a1, b0, b1;    // slot ranges of the two layers (b0 = b1 = 0 for a one-layer force)
  int32_t symmetric, i0, i1; // as in moog_force_t
  int32_t n_b;               // 0: one-layer force
  double p0, p1;
  int32_t pad[2];
};
static_assert(sizeof(FOp) == 64, "FOp is one 64-byte scalar load");

// The (force, layer a, layer b) combinations of a program in the order physics.py:96-108 visits them: writes the first `cap`
// of them to out[] and returns how many there are (cap = 0: only counts).
constexpr int moog_flatten_fops_into(const moog_program_t& p, FOp* out, int cap) {
  int n = 0;
  for (int fi = 0; fi < p.n_forces; ++fi) {
    const moog_force_t& F = p.forces[fi];
    for (int a = 0; a < F.n_a; ++a) {
      FOp op = {};
      op.fi = fi; op.kind = F.kind; op.symmetric = F.symmetric; op.i0 = F.i0; op.i1 = F.i1; op.p0 = F.p0; op.p1 = F.p1;
      op.a0 = p.layer_slot0[F.layers_a[a]]; op.a1 = op.a0 + p.layer_nslots[F.layers_a[a]];
      op.n_b = F.n_b;
      if (F.n_b == 0) { if (n < cap) out[n] = op; ++n; continue; }
      for (int b = 0; b < F.n_b; ++b) {
        op.b0 = p.layer_slot0[F.layers_b[b]]; op.b1 = op.b0 + p.layer_nslots[F.layers_b[b]];
        if (n < cap) out[n] = op;
        ++n;
      }
    }
  }
  return n;
}

constexpr int moog_count_fops(const moog_program_t& p) { return moog_flatten_fops_into(p, nullptr, 0); }

// The list as a value of fixed capacity (a constant when the program is one): n = the program's count, op[k] valid for
// k < min(n, CAP).
template <int CAP>
struct FOpList {
  FOp op[CAP > 0 ? CAP : 1];
  int n;
};
template <int CAP>
constexpr FOpList<CAP> moog_flatten_fops(const moog_program_t& p) {
  FOpList<CAP> l = {};
  l.n = moog_flatten_fops_into(p, l.op, CAP);
  return l;
}

// What the engine copies to device memory (KArgs::fops): the same function, run on the host.
inline std::vector<FOp> moog_flatten_forces(const moog_program_t* p) {
  std::vector<FOp> out((size_t)moog_count_fops(*p));
  moog_flatten_fops_into(*p, out.data(), (int)out.size());
  return out;
}
