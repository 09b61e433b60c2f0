// tfidf_weight.h -- the scalar rules of the TF-IDF calls (latok_idf_*, latok_tfidf_csr, latok_tfidf_utf8_bytes_batch): the idf of a
// column, the tf of a count, the division by a row's norm.  Plain C++: it compiles on the host (tests/helpers/tfidf_harness.cpp prints
// what it gives) and, under hipcc, on the device, where k_idf_weights and k_tfidf_rows (tfidf_kernels.hip) call nothing else.
//
//   tw_idf     idf = ln((n + s) / (df + s)) + 1 with s = 1 if smooth else 0, in double, rounded once to float32.  Without smoothing a
//              column that no document holds (df = 0) gets 0, where scikit-learn divides by zero.
//   tw_tf      tf = t, or with sublinear tf: sign(t) * (1 + ln|t|) for t != 0 and 0 for t = 0 (scikit-learn takes the logarithm of the
//              stored value: NaN for the negative and zero sums of alternate_sign; the two agree wherever it is defined).
//   tw_weight  w = tf * idf (one float32 product)
//   tw_term    what an entry adds to its row's norm: w * w (L2), |w| (L1)
//   tw_norm    the norm from the sum of the terms: sqrt (L2), the sum itself (L1)
//   tw_scale   out = w / N; a row whose norm is 0 holds only zeros and keeps them, and a zero weight stays +0: no NaN, no infinity.
#ifndef LATOK_TFIDF_WEIGHT_H
#define LATOK_TFIDF_WEIGHT_H
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define TW_FN __host__ __device__ __forceinline__
#else
#define TW_FN inline
#endif

constexpr int kTwSmoothIdf = 1, kTwSublinearTf = 2, kTwNormL1 = 4, kTwNormL2 = 8;   // = LATOK_TFIDF_* (include/latok_hip.h)
constexpr int kTwAllOpts = kTwSmoothIdf | kTwSublinearTf | kTwNormL1 | kTwNormL2;

TW_FN float tw_idf(int32_t df, int64_t n_docs, bool smooth) {
    const double s = smooth ? 1.0 : 0.0;
    if (!smooth && df <= 0) return 0.0f;
    return (float)(log(((double)n_docs + s) / ((double)df + s)) + 1.0);
}

TW_FN float tw_tf(int32_t t, bool sublinear) {
    if (!sublinear) return (float)t;
    if (t == 0) return 0.0f;
    const float a = 1.0f + logf(t < 0 ? -(float)t : (float)t);
    return t < 0 ? -a : a;
}

TW_FN float tw_weight(float tf, float idf) { return tf * idf; }

TW_FN float tw_term(float w, bool l2) { return l2 ? w * w : fabsf(w); }

TW_FN float tw_norm(float sum, bool l2) { return l2 ? sqrtf(sum) : sum; }

TW_FN float tw_scale(float w, float norm) { return (norm > 0.0f && w != 0.0f) ? w / norm : 0.0f; }

#endif
