// Node features of the batched graph (pyg_data/rigid_tasks_data.py:150-250 and the cloth / rope counterparts) as a device BODY, shared by
// the stand-alone launch (train_ops.hip: grl_build_features[_bump]) and the step's merged head launch (node_ops.hip: grl_step_head).
// Every 3-vector feature of every node type is "slice A of an observation group [- slice B]", gathered per node; one launch
// writes them all (the torch formulation is ~30 tiny split / index / stack / cat launches per network and step).
#pragma once
#include "grl_common.h"

namespace {

struct FeatDesc {
  float* out;            // output rows
  const float* a;        // term A: group tensor [B, a_stride], vector j of a sample at a + b*a_stride + a_off + 3*j (j = 0 if a_bcast)
  const float* b;        // optional term B (subtracted)
  const long long* gather;  // optional: node n -> b*n_per + j (compacted main node type); else n = b*n_per + j
  int out_row_stride, out_col;      // floats
  int rows_per_sample, row_off;     // > 0: output row = b*rows_per_sample + row_off + j (dense critic input); else row = n
  int n_nodes, n_per;
  int a_stride, a_off, a_bcast;
  int b_stride, b_off, b_bcast;
  int onehot_col, n_types;          // onehot_col >= 0: also write the node-type one-hot into columns [0, n_types)
};
constexpr int FEAT_MAX = 24;
struct FeatDescs { FeatDesc d[FEAT_MAX]; };

// ---- training noise (rigid_tasks_data.py:178-214, rope_tasks_data.py:168-186, pyg_data/utils.py:13-15): N(0, std^2) added to the actor's
// input vectors when train and training_noise.  Counter-based, drawn on the device (include/grl_hip.h grl_build_features_noise has the
// mapping): Philox4x32-10 (Salmon et al., SC'11) keyed by the 64-bit seed, counter = (element id lo, hi, draw lo, hi), Box-Muller on its
// four words, three of the four normals used.
GRL_DEVINL uint4 philox4x32_10(uint4 c, unsigned int k0, unsigned int k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const unsigned int lo0 = 0xD2511F53u * c.x, hi0 = __umulhi(0xD2511F53u, c.x);
    const unsigned int lo1 = 0xCD9E8D57u * c.z, hi1 = __umulhi(0xCD9E8D57u, c.z);
    c = make_uint4(hi1 ^ c.y ^ k0, lo1, hi0 ^ c.w ^ k1, lo0);
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;   // (the bump after the last round is dead)
  }
  return c;
}
// z = sqrt(-2 ln u1) (cos 2 pi u2, sin 2 pi u2), u1 = ((a >> 8) + 1) 2^-24 in (0, 1], u2 = (b >> 8) 2^-24 in [0, 1): both exact in fp32
GRL_DEVINL float2 box_muller(unsigned int a, unsigned int b) {
  const float u1 = (float)((a >> 8) + 1u) * 5.9604644775390625e-8f, u2 = (float)(b >> 8) * 5.9604644775390625e-8f;
  const float r = sqrtf(-2.f * logf(u1));
  return make_float2(r * cospif(2.f * u2), r * sinpif(2.f * u2));
}
// the three normals of element `elem` at draw `draw`
GRL_DEVINL float3 noise3(unsigned long long seed, unsigned long long draw, unsigned long long elem) {
  const uint4 r = philox4x32_10(make_uint4((unsigned int)elem, (unsigned int)(elem >> 32), (unsigned int)draw, (unsigned int)(draw >> 32)),
                                (unsigned int)seed, (unsigned int)(seed >> 32));
  const float2 z01 = box_muller(r.x, r.y), z23 = box_muller(r.z, r.w);
  return make_float3(z01.x, z01.y, z23.x);
}

// The noise arguments of a launch.  w[desc]: the descriptor's noise word (include/grl_hip.h): bit 0 = add the noise of (type, slot), bit 1 =
// add the noise of (type, slot 0) as well (corr under dist_as_pos: upstream computes it from the already noisy position); bits 8-15 slot,
// 16-23 n_slots, 24-31 type index, 32-63 the batch size B.  state: device {seed, draw, ticket} (uint64).
struct FeatNoise {
  unsigned long long w[FEAT_MAX];
  unsigned long long* state;
  float std;
  int n_blocks;   // the launch's feature workgroups: each takes one ticket
  int advance;    // 0: read the draw, leave it (the calibrating pass of policy.GNNGaussianPolicyDiag: the NEXT forward's draw)
};

// workgroup (bx of nbx) of descriptor `desc`; `first`: the one workgroup of the launch that advances the optional step count.
// NOISE: add training noise per the descriptor's word (above).  Every feature workgroup reads the draw at its start; the draw advances by one
// per launch, in stream order, through a LAST-WORKGROUP TICKET: after its nodes each workgroup takes a ticket (device-scope atomic behind a
// fence), the workgroup that takes the last one resets the ticket and stores draw + 1.  Every other workgroup has read the draw before it
// took its ticket, so no reader sees the new value; the next launch on the stream does.  (The step count's "block 0 bumps" cannot serve:
// the draw is read by every workgroup.)  NOISE = false is exactly the noise-free body.
template <bool NOISE>
GRL_DEVINL void build_features_body_t(const FeatDescs& all, int* __restrict__ bump, int bx, int nbx, int desc, bool first, const FeatNoise* nz) {
  // (optional) the optimizer's step count rides on this launch -- the first of a lane's recorded step: one thread advances it, every
  // later kernel of the lane (Adam) reads the new value; a separate one-element launch was ~6 us of every step's chain
  if (bump && first && threadIdx.x == 0) bump[0] += 1;
  const FeatDesc& f = all.d[desc];
  unsigned long long nw = 0, seed = 0, draw = 0;
  float sd = 0.f;
  if constexpr (NOISE) {
    __shared__ unsigned long long s_kd[2];
    if (threadIdx.x == 0) { s_kd[0] = nz->state[0]; s_kd[1] = nz->state[1]; }
    __syncthreads();
    nw = nz->w[desc]; seed = s_kd[0]; draw = s_kd[1]; sd = nz->std;
  }
  for (int n = bx * 256 + (int)threadIdx.x; n < f.n_nodes; n += nbx * 256) {
    const long long flat = f.gather ? f.gather[n] : (long long)n;
    const int b = (int)(flat / f.n_per), j = (int)(flat - (long long)b * f.n_per);
    float x = 0.f, y = 0.f, z = 0.f;
    if (f.a) {
      const float* p = f.a + (size_t)b * f.a_stride + f.a_off + (f.a_bcast ? 0 : 3 * j);
      x = p[0]; y = p[1]; z = p[2];
    }
    if (f.b) {
      const float* p = f.b + (size_t)b * f.b_stride + f.b_off + (f.b_bcast ? 0 : 3 * j);
      x -= p[0]; y -= p[1]; z -= p[2];
    }
    if constexpr (NOISE) {
      if (nw & 3ull) {
        // element id ((type * B + b) * n_per + j) * n_slots + slot: the NATURAL (sample, point) index, whatever the output row
        const unsigned long long slot = (nw >> 8) & 0xff, n_slots = (nw >> 16) & 0xff, type = (nw >> 24) & 0xff, B = nw >> 32;
        const unsigned long long e0 = ((type * B + (unsigned long long)b) * (unsigned long long)f.n_per + (unsigned long long)j) * n_slots;
        if (nw & 2ull) {   // the position slot's noise (its own Philox block, recomputed: no exchange between descriptors)
          const float3 q = noise3(seed, draw, e0);
          x += sd * q.x; y += sd * q.y; z += sd * q.z;
        }
        if (nw & 1ull) {
          const float3 q = noise3(seed, draw, e0 + slot);
          x += sd * q.x; y += sd * q.y; z += sd * q.z;
        }
      }
    }
    const size_t row = f.rows_per_sample > 0 ? (size_t)b * f.rows_per_sample + f.row_off + j : (size_t)n;
    float* o = f.out + row * f.out_row_stride;
    o[f.out_col] = x; o[f.out_col + 1] = y; o[f.out_col + 2] = z;
    if (f.onehot_col >= 0)
      for (int c = 0; c < f.n_types; ++c) o[c] = c == f.onehot_col ? 1.f : 0.f;
  }
  if constexpr (NOISE) {
    // (thread 0's load of the draw returned before the barrier above, so its ticket follows that read without a fence; the new draw and the
    // reset ticket are seen by the next launch through the kernel boundary.  No __threadfence: with a device-scope fence per workgroup the
    // stand-alone launch of 4096 frames took 81 us instead of 12)
    if (nz->advance && threadIdx.x == 0) {
      unsigned long long* ticket = nz->state + 2;
      if (atomicAdd(ticket, 1ull) == (unsigned long long)(nz->n_blocks - 1)) {
        atomicExch(ticket, 0ull);
        atomicExch(nz->state + 1, draw + 1ull);
      }
    }
  }
}
GRL_DEVINL void build_features_body(const FeatDescs& all, int* __restrict__ bump, int bx, int nbx, int desc, bool first) {
  build_features_body_t<false>(all, bump, bx, nbx, desc, first, nullptr);
}

// descs: HOST array of n_desc <= FEAT_MAX records of 18 8-byte words each (include/grl_hip.h grl_build_features); -> the largest node count
inline int feat_fill(FeatDescs& all, const long long* descs, int n_desc) {
  int max_nodes = 1;
  for (int i = 0; i < n_desc; ++i) {
    const long long* w = descs + 18 * i;
    FeatDesc& f = all.d[i];
    f.out = reinterpret_cast<float*>(w[0]);
    f.a = reinterpret_cast<const float*>(w[1]);
    f.b = reinterpret_cast<const float*>(w[2]);
    f.gather = reinterpret_cast<const long long*>(w[3]);
    f.out_row_stride = (int)w[4]; f.out_col = (int)w[5]; f.rows_per_sample = (int)w[6]; f.row_off = (int)w[7];
    f.n_nodes = (int)w[8]; f.n_per = (int)w[9];
    f.a_stride = (int)w[10]; f.a_off = (int)w[11]; f.a_bcast = (int)w[12];
    f.b_stride = (int)w[13]; f.b_off = (int)w[14]; f.b_bcast = (int)w[15];
    f.onehot_col = (int)w[16]; f.n_types = (int)w[17];
    if (f.n_nodes > max_nodes) max_nodes = f.n_nodes;
  }
  return max_nodes;
}
// noise: HOST array of n_desc noise words (include/grl_hip.h), state = device {seed, draw, ticket}
inline int feat_noise_fill(FeatNoise& nz, const long long* words, int n_desc, unsigned long long* state, float std, int n_blocks, int advance) {
  if (!words || !state || n_desc > FEAT_MAX) return -2;
  for (int i = 0; i < n_desc; ++i) nz.w[i] = (unsigned long long)words[i];
  nz.state = state; nz.std = std; nz.n_blocks = n_blocks; nz.advance = advance;
  return 0;
}

}  // namespace
