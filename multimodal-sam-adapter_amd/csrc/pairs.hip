// Panoptic quality on device: the intersections of (prediction segment, label segment) pairs as a hash table (mmsa_segment_pairs), and the matching of the
// pairs by IoU > 1/2 with the TP / FP / FN counts and the IoU sum per class and size (mmsa_eval_panoptic).  Integers only.
//
// The quantities.  Maps, codes, connectivity and roots are csrc/components.hip's.  A pixel takes part iff its own label code L is not
// MMSA_EVAL_IGNORE; area_g / area_p are the participating pixels of a label / prediction segment (planes 0 and 2 of mmsa_eval_segments' scratch); a HIT pixel
// has L < C and min(pred, C) == L, and inter(p, g) = the hit pixels with root_pred == p and root_label == g.  p and g MATCH iff 3 * inter > area_p + area_g
// (IoU > 1/2, strict, in integers); a segment has at most one match (two matches of one p would need inter1 + inter2 > area_p).
//
// The pair table (csrc/pair_table.h: the table, the in-wave reduction, the insert and its probe bound -- shared with csrc/track.hip).  Every hit pixel forms
//   key = ((b * HW + root_label) << 31) | root_pred          (< 2^62: B * H * W < 2^31)
// PAIR_WAVE_ROUNDS = 8 rounds of the in-wave reduction.  (Measured, profiles/panoptic.txt: a wave of a class map holds one to a few pairs, and 8 rounds
// equal 64 there -- 34 us for two 1024 x 1024 maps -- while 2 rounds leave whole edges to contend for one slot, 128 - 156 us; on a noise map, where a wave
// holds 64 keys and no round retires more than one lane, 8 rounds take 209 - 214 us against 226 - 232 us for 64.)
// PAIR_MAX_PROBES = 128.  The longest walk of a key in the measured tables is 2 slots for a class map (load 0.004), 7 for noise against noise (load 0.08)
// and 3 at load 0.42 (profiles/panoptic.txt), so a bound of 32 and one of 128 take the same time there; 128 keeps a margin for the loads near 1 that a small
// capacity= gives, and only ends the walk through a table that is too small after 128 CAS instead of `capacity`.
// The atomics are device-scope (HIP's default for atomicCAS / atomicAdd on global memory: performed at L2 / memory, coherent across XCDs); the table is
// READ by a later launch only.
#include "common.h"
#include "eval_hist.h"
#include "code_map.h"
#include "comp_shared.h"
#include "pair_table.h"

struct PairMaps {
  const unsigned char* pred;        // [B, H, W]
  const int* root_pred;             // [B, H, W]
  const int* root_label;
  int H, W, B;
};

// grid (cdiv(H * W, 256), B): a wave lies inside one image
__global__ __launch_bounds__(256) void segment_pairs_kernel(PairMaps m, EvalLabel ev, PairTable t) {
  const long HW = (long)m.H * m.W, i = (long)blockIdx.x * 256 + threadIdx.x, base = blockIdx.y * HW;
  bool pending = false;
  unsigned long long key = 0ull;
  if (i < HW) {
    const int l = label_code(ev, ev.lut, blockIdx.y, m.W, (int)i);
    pending = l < ev.C && min((int)m.pred[base + i], ev.C) == l;               // MMSA_EVAL_IGNORE = 255 > C: an ignored pixel is no hit
    const int rl = min(max(m.root_label[base + i], 0), (int)HW - 1);
    const int rp = min(max(m.root_pred[base + i], 0), (int)HW - 1);
    key = ((unsigned long long)(base + rl) << 31) | (unsigned long long)rp;
  }
  const int n = pair_wave_reduce(pending, key);
  if (n > 0) pair_insert(t, key, n);
}

extern "C" int mmsa_segment_pairs(const unsigned char* pred, const unsigned char* label, int Hl, int Wl, const unsigned char* lut, int C, const int* ymap,
                                  const int* xmap, const int* root_pred, const int* root_label, int B, int H, int W, int64_t* keys, int* counts, long capacity,
                                  int* overflow, hipStream_t stream) {
  const char* name = "segment_pairs";
  MMSA_CHECK_ARG(pred && label && lut && root_pred && root_label && overflow, "%s: pred, label, lut, root_pred, root_label and overflow are required", name);
  int rc = comp_check_size(name, B, H, W);
  if (rc) return rc;
  MMSA_CHECK_ARG(C >= 2 && C <= 254, "%s: %d classes; 2..254 are supported (a uint8 class map)", name, C);
  MMSA_CHECK_ARG(Hl > 0 && Wl > 0 && (long)Hl * Wl < (1l << 31), "%s: bad label size", name);
  MMSA_CHECK_ARG((ymap != NULL) == (xmap != NULL), "%s: ymap and xmap come together", name);
  MMSA_CHECK_ARG(ymap || (Hl == H && Wl == W), "%s: size mismatch: the label is %d x %d, the prediction %d x %d, and no ymap / xmap tables were given", name,
                 Hl, Wl, H, W);
  int log2cap = 0;
  rc = pair_check_table(name, keys, counts, capacity, &log2cap);
  if (rc) return rc;
  hipError_t e = hipMemsetAsync(keys, 0xff, (size_t)capacity * sizeof(int64_t), stream);
  MMSA_CHECK_ARG(e == hipSuccess, "%s: emptying the keys failed: %s", name, hipGetErrorString(e));
  rc = comp_zero(name, counts, (size_t)capacity * sizeof(int), stream);
  if (rc) return rc;
  const PairMaps m = {pred, root_pred, root_label, H, W, B};
  const EvalLabel ev = {label, lut, ymap, xmap, nullptr, Hl, Wl, C};
  const PairTable t = {(unsigned long long*)keys, counts, overflow, log2cap};
  hipLaunchKernelGGL(segment_pairs_kernel, dim3((unsigned)cdiv((long)H * W, 256l), B), dim3(256), 0, stream, m, ev, t);
  MMSA_CHECK_LAUNCH("segment_pairs");
  return MMSA_OK;
}

// ---- matching and counting
struct PanopticMaps {
  const unsigned char* pred;        // [B, H, W]
  const int* root_pred;             // [B, H, W]
  const int* root_label;
  const int* planes;                // [4, B, H, W] as mmsa_eval_segments left them: area0, hit0, area1, hit1 at the root pixels
  int* match;                       // [2, B, H, W]: at a label root its prediction root, at a prediction root its label root, -1 elsewhere
  int H, W, B;
};

// the cell [c, s] of pq_counts' slot (4 integers: TP, FP, FN, IoU sum), as an index of its first integer
__device__ __forceinline__ int pq_cell(int c, int area) { return (c * COMP_SIZE_BUCKETS + comp_size_bucket(area)) * 4; }

// grid cdiv(capacity, 256): a lane per slot of the table.  pq [n_slots, C, 24, 4]; n_slots * C * 96 < 2^31 (checked by the entry)
__global__ __launch_bounds__(256) void panoptic_match_kernel(PanopticMaps m, EvalLabel ev, EvalSlots es, const unsigned long long* __restrict__ keys,
                                                             const int* __restrict__ counts, long capacity) {
  const long j = (long)blockIdx.x * 256 + threadIdx.x, HW = (long)m.H * m.W, plane = (long)m.B * HW;
  int bin = -1;
  unsigned long long q = 0ull;
  if (j < capacity) {
    const unsigned long long key = keys[j];
    const long g = (long)(key >> 31), rp = (long)(key & 0x7fffffffull);       // a table from elsewhere cannot send anything outside the planes:
    const long inter = counts[j];
    if (key != PAIR_EMPTY && g < plane && rp < HW && inter > 0) {              // an empty key has g = 2^33 - 1 >= plane
      const int b = (int)(g / HW), rl = (int)(g - (long)b * HW);
      const long area_g = m.planes[g], area_p = m.planes[2 * plane + (long)b * HW + rp];
      if (3 * inter > area_p + area_g && inter <= area_g && inter <= area_p) {
        m.match[g] = (int)rp;
        m.match[plane + (long)b * HW + rp] = rl;
        const int c = label_code(ev, ev.lut, b, m.W, rl);
        if (c < ev.C) {
          bin = (es.s[b] * ev.C * COMP_SIZE_BUCKETS * 4) + pq_cell(c, (int)area_g);
          q = ((unsigned long long)inter << 24) / (unsigned long long)(area_p + area_g - inter);      // inter < 2^31: exact in 64 bits; union >= inter > 0
        }
      }
    }
  }
  seg_count_add(ev.counts, bin);                                               // TP
  if (bin >= 0) atomicAdd(&ev.counts[bin + 3], q);
}

// grid (cdiv(H * W, 256), B): every root pixel without a match adds its segment: a label root one FN, a prediction root one FP
__global__ __launch_bounds__(256) void panoptic_count_kernel(PanopticMaps m, EvalLabel ev, EvalSlots es) {
  const long HW = (long)m.H * m.W, i = (long)blockIdx.x * 256 + threadIdx.x, base = blockIdx.y * HW, plane = (long)m.B * HW;
  const int C = ev.C, b = blockIdx.y;
  unsigned long long* slot = ev.counts + (long)es.s[b] * C * COMP_SIZE_BUCKETS * 4;
  int fn = -1, fp = -1;
  if (i < HW) {
    if (m.root_label[base + i] == (int)i && m.match[base + i] < 0) {
      const int a = m.planes[base + i];
      if (a > 0) {
        const int c = label_code(ev, ev.lut, b, m.W, (int)i);
        if (c < C) fn = pq_cell(c, a) + 2;
      }
    }
    if (m.root_pred[base + i] == (int)i && m.match[plane + base + i] < 0) {
      const int a = m.planes[2 * plane + base + i];
      const int c = min((int)m.pred[base + i], C);
      if (a > 0 && c < C) fp = pq_cell(c, a) + 1;
    }
  }
  seg_count_add(slot, fn);
  seg_count_add(slot, fp);
}

extern "C" int mmsa_eval_panoptic(const unsigned char* pred, const unsigned char* label, int B, int H, int W, int Hl, int Wl, const unsigned char* lut, int C,
                                  const int* ymap, const int* xmap, const int* slots /* HOST [B] */, int n_slots, const int* root_pred, const int* root_label,
                                  const int* planes, const int64_t* keys, const int* counts, long capacity, int* match, int64_t* pq_counts,
                                  hipStream_t stream) {
  const char* name = "eval_panoptic";
  MMSA_CHECK_ARG(pred && root_pred && root_label && planes && match, "%s: pred, root_pred, root_label, planes and match are required", name);
  EvalSlots es;
  int rc = eval_check(name, label, B, H, W, Hl, Wl, lut, C, ymap, xmap, slots, n_slots, pq_counts, es, 254, "a uint8 class map");
  if (rc) return rc;
  rc = comp_check_size(name, B, H, W);
  if (rc) return rc;
  MMSA_CHECK_ARG((long)n_slots * C * COMP_SIZE_BUCKETS * 4 < (1l << 31), "%s: %d slots of %d classes: a cell is indexed in 32 bits (n_slots * C * 96 < 2^31)",
                 name, n_slots, C);
  int log2cap = 0;
  rc = pair_check_table(name, keys, counts, capacity, &log2cap);
  if (rc) return rc;
  const hipError_t e = hipMemsetAsync(match, 0xff, (size_t)2 * B * H * W * sizeof(int), stream);
  MMSA_CHECK_ARG(e == hipSuccess, "%s: clearing the match planes failed: %s", name, hipGetErrorString(e));
  const PanopticMaps m = {pred, root_pred, root_label, planes, match, H, W, B};
  const EvalLabel ev = {label, lut, ymap, xmap, (unsigned long long*)pq_counts, Hl, Wl, C};
  hipLaunchKernelGGL(panoptic_match_kernel, dim3((unsigned)cdiv(capacity, 256l)), dim3(256), 0, stream, m, ev, es, (const unsigned long long*)keys, counts,
                     capacity);
  hipLaunchKernelGGL(panoptic_count_kernel, dim3((unsigned)cdiv((long)H * W, 256l), B), dim3(256), 0, stream, m, ev, es);
  MMSA_CHECK_LAUNCH("eval_panoptic");
  return MMSA_OK;
}
