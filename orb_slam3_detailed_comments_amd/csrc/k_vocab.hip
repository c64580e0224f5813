// k_vocab.hip — DBoW2 vocabulary transform: what Frame::ComputeBoW / KeyFrame::ComputeBoW
// (src/Frame.cc:984-997) ask of ORBVocabulary::transform(features, BowVector&, FeatureVector&, levelsup = 4)
// (Thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h:1127-1195), on the device:
//   k_voc_descend   the per-feature tree descent (TemplatedVocabulary.h:1218-1259): at every level the child with the smallest
//                   Hamming distance (FORB::distance, FORB.cpp:81-101), first child on ties (strict `d < best_d`), until a node
//                   without children; records the word id, the word weight and the ancestor at level L - levelsup.
//                   A group of 16 lanes serves one feature (one child per lane and trip; k = 10 in ORBvoc), 4 features per wave;
//                   the children of a node sit in consecutive slots so the group reads one contiguous 32*k-byte run.
//   k_voc_assemble  one workgroup per image: BowVector (std::map<WordId, WordValue>: ascending word ids, value accumulated by
//                   addWeight in feature order, then L1/L2-normalised in id order, BowVector.cpp:27-84) and FeatureVector
//                   (std::map<NodeId, vector<unsigned>>: ascending node ids, feature indices in insertion order) as sorted
//                   arrays; bitonic sort of (id << 16 | feature) keys in LDS, run detection with a workgroup scan, and the
//                   order-dependent double-precision sums done sequentially by one thread exactly as the map iteration does.
// Key frame database (KeyFrameDatabase, src/KeyFrameDatabase.cc; host side in orbv_api.cpp: orbv_db_*): one record per add, in add order,
// with its sorted BowVector in a CSR arena.  Three launches per batch of Q queries:
//   k_kfdb_count    one wave per (record, query): the words the record shares with the query (binary search in the query's sorted ids in
//                   LDS) times the record's multiplicity (duplicate adds fold into the earliest; the others carry 0), and the position in
//                   the query of the first shared word.  This is what the inverted-file walk of Detect*Candidates counts per key frame.
//   k_kfdb_order    one workgroup per query: drops excluded keys, the maximum and minCommonWords = (int)(max * 0.8f), and a stable
//                   counting sort of the sharing records on the first shared position (records are in add order, so this is the order in
//                   which the walk first meets them: word by word, each word's list in add order).
//   k_kfdb_score    one wave per scored key: ScoringObject::score (Thirdparty/DBoW2/DBoW2/ScoringObject.cpp), one term per common word, added
//                   in ascending word order in fp64 exactly as the reference's loop does (no reassociation, no contraction).
#include "orbx_types.h"
#include "orbx_block.h"

namespace orbx {

constexpr int kVocGroup = 16;      // lanes per feature in k_voc_descend

// grid (ceil(n_total / 16)), 256 threads.  Features of image b are fdesc[(b*cap + i)*4 .. +3], i < n_feat[b] (n_feat == nullptr:
// one image with n_fixed features).  Outputs are indexed like the features.
__global__ void __launch_bounds__(256) k_voc_descend(const unsigned long long* __restrict__ fdesc, const int* __restrict__ n_feat, int n_fixed,
                                                     int cap, int B, const unsigned long long* __restrict__ slot_desc,
                                                     const VocSlot* __restrict__ slots, const double* __restrict__ slot_weight,
                                                     int root_children, int nid_level, unsigned* __restrict__ out_word,
                                                     unsigned* __restrict__ out_node, double* __restrict__ out_weight) {
    const int g = (int)((blockIdx.x * 256u + threadIdx.x) / kVocGroup), sub = (int)(threadIdx.x & (kVocGroup - 1));
    const int b = g / cap, i = g - b * cap;
    // whole groups leave together (g is uniform inside a group), so the width-16 shuffles below never wait for a missing lane
    if (b >= B) return;
    const int n = n_feat ? n_feat[b] : n_fixed;
    if (i >= n) return;
    const unsigned long long* f = fdesc + 4 * ((size_t)b * cap + i);
    const unsigned long long f0 = f[0], f1 = f[1], f2 = f[2], f3 = f[3];
    int cs = 0, cc = root_children, level = 0, slot = -1;
    unsigned nid = 0;
    bool have_nid = nid_level <= 0;          // "if(nid_level <= 0 && nid != NULL) *nid = 0; // root"
    // the loop runs while any group of the wave still descends (groups whose leaf is shallower idle with cc == 0), which keeps the
    // width-16 exchanges convergent
    while (__ballot(cc > 0) != 0ull) {
        level++;
        unsigned best = 0xFFFFFFFFu;         // dist << 8 | child: minimum = smallest distance, first child on ties
        for (int c0 = 0; c0 < cc; c0 += kVocGroup) {
            const int c = c0 + sub;
            unsigned key = 0xFFFFFFFFu;
            if (c < cc) {
                const unsigned long long* d = slot_desc + 4 * (size_t)(cs + c);
                const int dist = __popcll(f0 ^ d[0]) + __popcll(f1 ^ d[1]) + __popcll(f2 ^ d[2]) + __popcll(f3 ^ d[3]);
                key = ((unsigned)dist << 8) | (unsigned)c;
            }
            best = key < best ? key : best;
        }
#pragma unroll
        for (int d = kVocGroup / 2; d >= 1; d >>= 1) { const unsigned o = __shfl_xor(best, d, kVocGroup); best = o < best ? o : best; }
        if (cc > 0) {
            slot = cs + (int)(best & 0xFFu);
            const VocSlot s = slots[slot];
            if (level == nid_level) { nid = (unsigned)s.node_id; have_nid = true; }
            cs = s.child_start; cc = s.child_cnt;
        }
    }
    if (sub == 0) {
        const size_t o = (size_t)b * cap + i;
        if (slot < 0) { out_word[o] = 0; out_node[o] = 0; out_weight[o] = 0.0; return; }   // empty vocabulary
        const VocSlot s = slots[slot];
        out_word[o] = (unsigned)s.word_id;
        // a leaf above level L - levelsup: the reference leaves *nid untouched (an uninitialised local, TemplatedVocabulary.h:1150);
        // here that case yields the leaf itself
        out_node[o] = have_nid ? nid : (unsigned)s.node_id;
        out_weight[o] = slot_weight[slot];
    }
}

// in-LDS bitonic sort of P (power of two) 64-bit keys, ascending; all 256 threads
__device__ __forceinline__ void bitonic_sort_u64(unsigned long long* key, int P, int tid) {
    for (int k = 2; k <= P; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = tid; t < P; t += 256) {
                const int p = t ^ j;
                if (p > t) {
                    const unsigned long long a = key[t], b2 = key[p];
                    const bool up = (t & k) == 0;
                    if ((a > b2) == up) { key[t] = b2; key[p] = a; }
                }
            }
            __syncthreads();
        }
}

// run starts of the sorted keys (id = key >> 16): ids[u], start[u] for every distinct id, start[nu] = nvalid; returns nu (all threads)
__device__ __forceinline__ int emit_runs(const unsigned long long* key, int nvalid, unsigned* __restrict__ ids, int* __restrict__ start,
                                         int tid, unsigned long long* scan_scratch) {
    int base = 0;
    for (int i0 = 0; i0 < nvalid; i0 += 256) {
        const int i = i0 + tid;
        int flag = 0;
        if (i < nvalid) flag = (i == 0) || ((key[i] >> 16) != (key[i - 1] >> 16));
        unsigned long long tot;
        const int ex = (int)block_excl_scan<unsigned long long>((unsigned long long)flag, &tot, scan_scratch);
        if (flag) { ids[base + ex] = (unsigned)(key[i] >> 16); start[base + ex] = i; }
        base += (int)tot;
    }
    if (tid == 0) start[base] = nvalid;
    return base;
}

// grid (B), 256 threads, dynamic LDS = P * 8 bytes (P = pow2 >= max features per image).
// weighting: 0 TF_IDF, 1 TF, 2 IDF, 3 BINARY;  norm: 0 none, 1 L1, 2 L2  (BowVector.h:29-50, ScoringObject.h:74-89)
// Per image b (regions of `cap` entries): bow_id/bow_val/[n_out[2b]], fv_node/fv_start(cap+1)/fv_feat/[n_out[2b+1]];
// bow_start: scratch, cap+1 ints per image.
// orbv_transform_rig_extracted: the rows of rig frame b as the rig Frame's mDescriptors holds them (src/Frame.cc:1514, cv::vconcat): the descriptors
// of left image b (camera 1) then those of right image b (camera 2), at out[(b * 2 cap + i) * 4]; n_out[b] = Nleft + Nright.  grid (ceil(2 cap / 256), B).
__global__ void __launch_bounds__(256) k_voc_gather_rig(const unsigned long long* __restrict__ desc_l, const int* __restrict__ n_l,
                                                        const unsigned long long* __restrict__ desc_r, const int* __restrict__ n_r, int cap, int B,
                                                        unsigned long long* __restrict__ out, int* __restrict__ n_out) {
    const int b = (int)blockIdx.y, i = (int)(blockIdx.x * 256u + threadIdx.x);
    if (b >= B) return;
    const int nl = imin(n_l[b], cap), nr = imin(n_r[b], cap);
    if (i == 0) n_out[b] = nl + nr;
    if (i >= nl + nr) return;
    const unsigned long long* s = i < nl ? desc_l + 4 * ((size_t)b * cap + i) : desc_r + 4 * ((size_t)b * cap + (i - nl));
    unsigned long long* d = out + 4 * ((size_t)b * 2 * cap + i);
    d[0] = s[0]; d[1] = s[1]; d[2] = s[2]; d[3] = s[3];
}

__global__ void __launch_bounds__(256) k_voc_assemble(const unsigned* __restrict__ word, const unsigned* __restrict__ node,
                                                      const double* __restrict__ weight, const int* __restrict__ n_feat, int n_fixed, int cap,
                                                      int P, int weighting, int norm, unsigned* __restrict__ bow_id,
                                                      double* __restrict__ bow_val, int* __restrict__ bow_start,
                                                      unsigned* __restrict__ fv_node, int* __restrict__ fv_start,
                                                      unsigned* __restrict__ fv_feat, int* __restrict__ n_out) {
    ORBX_DYN_SMEM(smem);
    __shared__ unsigned long long s_scan[20];
    __shared__ int s_nvalid;
    __shared__ double s_norm;
    unsigned long long* key = (unsigned long long*)smem;
    const int tid = (int)threadIdx.x, b = (int)blockIdx.x;
    const int n = n_feat ? n_feat[b] : n_fixed;
    const size_t off = (size_t)b * cap, offs = (size_t)b * (cap + 1);
    const unsigned* w_ = word + off; const unsigned* nd_ = node + off; const double* wt_ = weight + off;
    const unsigned long long kEmpty = ~0ull;
    for (int pass = 0; pass < 2; pass++) {
        // "if(w > 0) // not stopped": stopped features enter neither vector
        if (tid == 0) s_nvalid = 0;
        __syncthreads();
        int mine = 0;
        for (int i = tid; i < P; i += 256) {
            unsigned long long k = kEmpty;
            if (i < n && wt_[i] > 0) { k = ((unsigned long long)(pass == 0 ? w_[i] : nd_[i]) << 16) | (unsigned long long)i; mine++; }
            key[i] = k;
        }
        if (mine) atomicAdd(&s_nvalid, mine);
        __syncthreads();
        bitonic_sort_u64(key, P, tid);
        const int nvalid = s_nvalid;
        if (pass == 0) {
            const int nu = emit_runs(key, nvalid, bow_id + off, bow_start + offs, tid, s_scan);
            __syncthreads();
            // value of each word: addWeight adds w once per feature in feature order (TF_IDF / TF); addIfNotExist keeps the first (IDF / BINARY)
            for (int u = tid; u < nu; u += 256) {
                const int s = bow_start[offs + u], e = bow_start[offs + u + 1];
                const double w = wt_[(int)(key[s] & 0xFFFFu)];
                double v = w;
                if (weighting <= 1) for (int t = s + 1; t < e; t++) v = v + w;
                bow_val[off + u] = v;
            }
            __syncthreads();
            if (weighting <= 1 && norm == 0 && nu > 0) {           // "unnecessary when normalizing": vit->second /= nd
                const double ndv = (double)nu;
                for (int u = tid; u < nu; u += 256) bow_val[off + u] = bow_val[off + u] / ndv;
            }
            if (norm != 0) {                                        // BowVector::normalize, in ascending id order
                if (tid == 0) {
                    double acc = 0.0;
                    if (norm == 1) for (int u = 0; u < nu; u++) acc = acc + fabs(bow_val[off + u]);
                    else { for (int u = 0; u < nu; u++) acc = acc + bow_val[off + u] * bow_val[off + u]; acc = sqrt(acc); }
                    s_norm = acc;
                }
                __syncthreads();
                const double nv = s_norm;
                if (nv > 0.0) for (int u = tid; u < nu; u += 256) bow_val[off + u] = bow_val[off + u] / nv;
            }
            if (tid == 0) n_out[2 * b] = nu;
        } else {
            const int nu = emit_runs(key, nvalid, fv_node + off, fv_start + offs, tid, s_scan);
            for (int i = tid; i < nvalid; i += 256) fv_feat[off + i] = (unsigned)(key[i] & 0xFFFFu);
            if (tid == 0) n_out[2 * b + 1] = nu;
        }
        __syncthreads();
    }
}

// ---- key frame database ----
// position of w in the ascending ids qw[0, nq), or -1
__device__ __forceinline__ int kfdb_find(const unsigned* qw, int nq, unsigned w) {
    int lo = 0, hi = nq;
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (qw[mid] < w) lo = mid + 1; else hi = mid; }
    return (lo < nq && qw[lo] == w) ? lo : -1;
}

// grid (ceil(R / 32), Q), 256 threads, dynamic LDS = 4 * (largest query) bytes.  cnt / firstpos [Q][R]: 0 / 0xFFFFFFFF for a record that
// shares nothing, is erased or is a later duplicate (rmult 0)
__global__ void __launch_bounds__(256) k_kfdb_count(const unsigned* __restrict__ ids, const long long* __restrict__ rstart, const int* __restrict__ rn,
                                                    const int* __restrict__ rmult, int R, KfdbQuerySet qs, int* __restrict__ cnt, int* __restrict__ firstpos) {
    ORBX_DYN_SMEM(smem);
    unsigned* qw = (unsigned*)smem;
    const int tid = (int)threadIdx.x, lane = lane_id(), wave = tid >> 6, q = (int)blockIdx.y;
    const int nq = qs.n[(size_t)q * qs.n_step];
    const unsigned* src = qs.ids + (qs.start ? (size_t)qs.start[q] : (size_t)q * qs.stride);
    for (int i = tid; i < nq; i += 256) qw[i] = src[i];
    __syncthreads();
    const int rb = (int)blockIdx.x * kKfdbRecsPerBlock, re = imin(R, rb + kKfdbRecsPerBlock);
    for (int r = rb + wave; r < re; r += 4) {
        const int m = rmult[r];
        int c = 0;
        unsigned f = 0xFFFFFFFFu;
        if (m > 0 && nq > 0) {
            const long long s = rstart[r];
            const int n = rn[r];
            for (int i0 = 0; i0 < n; i0 += 64) {
                const int i = i0 + lane;
                if (i < n) {
                    const int p = kfdb_find(qw, nq, ids[s + i]);
                    if (p >= 0) { c++; f = (unsigned)p < f ? (unsigned)p : f; }
                }
            }
            c = wave_sum(c);
            f = wave_min_u32(f);
        }
        if (lane == 0) { cnt[(size_t)q * R + r] = c * m; firstpos[(size_t)q * R + r] = (int)f; }
    }
}

// grid (Q), nw * 64 threads (nw <= 16), dynamic LDS = 4 * nw * (largest query) bytes: one row of bin counters per wave.
// Excluded records (xrec[xstart[q] .. xstart[q+1])) are zeroed in cnt first.  Wave w owns records [w * seg, (w + 1) * seg): it counts
// their first positions into its row, the rows become exclusive offsets (bin-major, then wave), and every wave places its records in
// record order, 64 at a time, ranking equal bins by lane.  head[4q] = sharing keys, head[4q + 1] = minCommonWords, head[4q + 2] = scored.
__global__ void __launch_bounds__(1024) k_kfdb_order(int* __restrict__ cnt, const int* __restrict__ firstpos, const unsigned long long* __restrict__ rkey, int R,
                                                     const int* __restrict__ qn, int qn_step, const int* __restrict__ xstart, const int* __restrict__ xrec,
                                                     int score_all, int* __restrict__ order, KfdbHit* __restrict__ hits, int* __restrict__ slist,
                                                     int* __restrict__ head) {
    ORBX_DYN_SMEM(smem);
    __shared__ int s_red[16];
    __shared__ int s_scan[20];
    __shared__ int s_nscored;
    int* hist = (int*)smem;
    const int tid = (int)threadIdx.x, nt = (int)blockDim.x, nw = nt >> 6, wave = tid >> 6, lane = lane_id(), q = (int)blockIdx.x;
    const int nq = qn[(size_t)q * qn_step];
    int* c = cnt + (size_t)q * R;
    const int* fp = firstpos + (size_t)q * R;
    if (xstart) for (int i = xstart[q] + tid; i < xstart[q + 1]; i += nt) c[xrec[i]] = 0;
    for (int i = tid; i < nw * nq; i += nt) hist[i] = 0;
    if (tid == 0) s_nscored = 0;
    __syncthreads();
    const int seg = (R + nw - 1) / nw, r0 = imin(R, wave * seg), r1 = imin(R, r0 + seg);
    int* row = hist + (size_t)wave * nq;
    int mx = 0;
    for (int r = r0 + lane; r < r1; r += 64) {
        const int v = c[r];
        if (v > 0) { atomicAdd(&row[fp[r]], 1); mx = v > mx ? v : mx; }
    }
    for (int d = 32; d >= 1; d >>= 1) { const int o2 = __shfl_xor(mx, d); mx = o2 > mx ? o2 : mx; }
    if (lane == 0) s_red[wave] = mx;
    __syncthreads();
    mx = 0;
    for (int w = 0; w < nw; w++) mx = s_red[w] > mx ? s_red[w] : mx;
    int carry = 0;
    for (int b0 = 0; b0 < nq; b0 += nt) {
        const int b = b0 + tid;
        int tot = 0;
        if (b < nq) for (int w = 0; w < nw; w++) tot += hist[(size_t)w * nq + b];
        int total;
        const int ex = block_excl_scan<int>(tot, &total, s_scan);
        if (b < nq) {
            int run = carry + ex;
            for (int w = 0; w < nw; w++) { const int t = hist[(size_t)w * nq + b]; hist[(size_t)w * nq + b] = run; run += t; }
        }
        carry += total;
    }
    __syncthreads();
    const int minc = (int)((float)mx * 0.8f);          // "int minCommonWords = maxCommonWords * 0.8f"
    if (tid == 0) { head[4 * q] = carry; head[4 * q + 1] = minc; }
    int* o = order + (size_t)q * R;
    KfdbHit* hq = hits + (size_t)q * R;
    int* sl = slist + (size_t)q * R;
    for (int base = r0; base < r1; base += 64) {
        const int r = base + lane;
        const int v = r < r1 ? c[r] : 0;
        const int bin = v > 0 ? fp[r] : -1;
        unsigned long long act = __ballot(v > 0 ? 1 : 0);
        if (act == 0ull) continue;
        int rank = 0;
        bool last = true;
        while (act) {
            const int j = __ffsll((unsigned long long)act) - 1;
            act &= act - 1ull;
            const int bj = __shfl(bin, j);
            if (bin >= 0 && bj == bin) { if (j < lane) rank++; else if (j > lane) last = false; }
        }
        int pos = 0;
        if (bin >= 0) pos = row[bin] + rank;
        ORBX_WAVE_SYNC();
        if (bin >= 0 && last) row[bin] = pos + 1;
        ORBX_WAVE_SYNC();
        if (bin >= 0) {
            o[pos] = r;
            const int sc = (score_all || v > minc) ? 1 : 0;
            KfdbHit h; h.key = rkey[r]; h.score = 0.0; h.words = v; h.scored = sc;
            hq[pos] = h;
            if (sc) sl[atomicAdd(&s_nscored, 1)] = pos;
        }
    }
    __syncthreads();
    if (tid == 0) head[4 * q + 2] = s_nscored;
}

// grid (S, Q), 256 threads, dynamic LDS = 12 * (largest query) bytes.  scoring = DBoW2::ScoringType (KL is refused by the host).
// Products and sums are written as __dmul_rn / __dadd_rn / __dsub_rn so that nothing is contracted into an FMA; the divisions and square
// roots are the correctly rounded IEEE operations the host's are.
__global__ void __launch_bounds__(256) k_kfdb_score(const unsigned* __restrict__ ids, const double* __restrict__ vals, const long long* __restrict__ rstart,
                                                    const int* __restrict__ rn, KfdbQuerySet qs, const int* __restrict__ order, const int* __restrict__ slist,
                                                    const int* __restrict__ head, KfdbHit* __restrict__ hits, int R, int scoring) {
    ORBX_DYN_SMEM(smem);
    const int tid = (int)threadIdx.x, lane = lane_id(), wave = tid >> 6, q = (int)blockIdx.y;
    const int ns = head[4 * q + 2];
    if ((int)blockIdx.x * 4 >= ns) return;                 // the whole workgroup leaves together
    const int nq = qs.n[(size_t)q * qs.n_step];
    const size_t qo = qs.start ? (size_t)qs.start[q] : (size_t)q * qs.stride;
    double* qv = (double*)smem;
    unsigned* qw = (unsigned*)(qv + nq);
    for (int i = tid; i < nq; i += 256) { qw[i] = qs.ids[qo + i]; qv[i] = qs.vals[qo + i]; }
    __syncthreads();
    for (int k = (int)blockIdx.x * 4 + wave; k < ns; k += (int)gridDim.x * 4) {
        const int pos = slist[(size_t)q * R + k], r = order[(size_t)q * R + pos];
        const long long s = rstart[r];
        const int n = rn[r];
        double acc = 0.0;
        for (int i0 = 0; i0 < n; i0 += 64) {
            const int i = i0 + lane;
            int hit = 0;
            double t = 0.0;
            if (i < n) {
                const int p = kfdb_find(qw, nq, ids[s + i]);
                if (p >= 0) {
                    const double vi = qv[p], wi = vals[s + i];
                    hit = 1;
                    switch (scoring) {
                        case 0: t = __dsub_rn(__dsub_rn(fabs(__dsub_rn(vi, wi)), fabs(vi)), fabs(wi)); break;     // L1: fabs(vi - wi) - fabs(vi) - fabs(wi)
                        case 2: { const double sv = __dadd_rn(vi, wi);                                          // chi^2: vi * wi / (vi + wi), if vi + wi != 0
                                  if (sv != 0.0) t = __dmul_rn(vi, wi) / sv; else hit = 0; } break;
                        case 4: t = sqrt(__dmul_rn(vi, wi)); break;                                             // Bhattacharyya: sqrt(vi * wi)
                        default: t = __dmul_rn(vi, wi); break;                                                  // L2, dot product: vi * wi
                    }
                }
            }
            unsigned long long m = __ballot(hit);
            while (m) {                                    // the terms of this chunk in ascending word order, one after the other
                const int j = __ffsll((unsigned long long)m) - 1;
                m &= m - 1ull;
                acc = __dadd_rn(acc, __shfl(t, j));
            }
        }
        double score = acc;
        if (scoring == 0) score = -acc / 2.0;                                         // "score = -score/2.0"
        else if (scoring == 1) score = acc >= 1.0 ? 1.0 : __dsub_rn(1.0, sqrt(__dsub_rn(1.0, acc)));   // rounding errors; 1 - sqrt(1 - score)
        else if (scoring == 2) score = __dmul_rn(2.0, acc);                           // "score = 2. * score"
        if (lane == 0) hits[(size_t)q * R + pos].score = score;
    }
}

}  // namespace orbx
