// The arithmetic of the two-window t-statistic event detector, stated once for the host detector (event_detect.cpp) and for the device
// kernels (signal_prep.hip): the t-statistic of one window, the peak detector's step, an event's mean and deviation, and the sample clock's
// uint32 indices.  Every operation is IEEE fp64; both users compile without contraction into fma, so that both round alike.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define RV_HD __host__ __device__
#else
#define RV_HD
#endif

namespace evcore {

constexpr double kFltMin = 1.17549435e-38, kFltMax = 3.40282347e+38;   // event_detector.py:10-11

struct Detector {
  double threshold; int window_length;
  uint32_t masked_to; int64_t peak_pos; double peak_value; bool valid_peak;
};

RV_HD inline Detector make_detector(double threshold, int window_length) {
  return Detector{threshold, window_length, 0u, -1, kFltMax, false};
}

// The clock after sample k (0-based) has been added: t = k + 2, the last ring slot written holds the sums of t - 1 = k + 1 samples
RV_HD inline uint32_t buf_mid_of(uint32_t t, int buf_len) { return (uint32_t)(t - (uint32_t)(buf_len / 2) - 1u); }
RV_HD inline uint32_t evt_en_of(uint32_t buf_mid, int w1) { return (uint32_t)(buf_mid - (uint32_t)w1 + 1u); }
RV_HD inline bool tstat_is_zero(uint32_t t, int w) { return (int64_t)t <= 2 * (int64_t)w || w < 2; }

// The ring slots _compute_tstat reads (:109-147), as the uint32 clock wraps them
struct TstatSlots { uint32_t i, st, en; };
RV_HD inline TstatSlots tstat_slots(uint32_t buf_mid, int w, int buf_len) {
  return TstatSlots{buf_mid % (uint32_t)buf_len, (uint32_t)(buf_mid - (uint32_t)w) % (uint32_t)buf_len,
                    (uint32_t)(buf_mid + (uint32_t)w) % (uint32_t)buf_len};
}

// _compute_tstat :109-147 from the running sums in the three slots
RV_HD inline double tstat(double s_st, double q_st, double s_i, double q_i, double s_en, double q_en, int w) {
  const double wf = (double)w;
  const double sum1 = s_i - s_st, sumsq1 = q_i - q_st;
  const double sum2 = s_en - s_i, sumsq2 = q_en - q_i;
  const double mean1 = sum1 / wf, mean2 = sum2 / wf;
  double var = sumsq1 / wf - mean1 * mean1 + sumsq2 / wf - mean2 * mean2;
  var = fmax(var, kFltMin);
  return fabs(mean2 - mean1) / sqrt(var / wf);
}

// _detect_peak :149-187; ld: the long detector, which a short detector's peak masks
RV_HD inline bool detect_peak(double cur, Detector& d, Detector& ld, bool is_short, uint32_t buf_mid, double peak_height) {
  if (d.masked_to >= buf_mid) return false;
  if (d.peak_pos == -1) {
    if (cur < d.peak_value) d.peak_value = cur;
    else if (cur - d.peak_value > peak_height) { d.peak_value = cur; d.peak_pos = (int32_t)buf_mid; }
  } else {
    if (cur > d.peak_value) { d.peak_value = cur; d.peak_pos = (int32_t)buf_mid; }
    if (is_short && d.peak_value > d.threshold) {
      ld.masked_to = (uint32_t)(d.peak_pos + d.window_length);
      ld.peak_pos = -1; ld.peak_value = kFltMax; ld.valid_peak = false;
    }
    if (d.peak_value - cur > peak_height && d.peak_value > d.threshold) d.valid_peak = true;
    if (d.valid_peak && (double)((int64_t)buf_mid - d.peak_pos) > d.window_length / 2.0) {
      d.peak_pos = -1; d.peak_value = cur; d.valid_peak = false;
      return true;
    }
  }
  return false;
}

// _create_event :189-210: the length of the event that ends at evt_en (an event is made only when it is >= kFltMin) ...
RV_HD inline double event_len(uint32_t evt_en, int64_t evt_st) { return (double)((int64_t)evt_en - evt_st); }
// ... and its mean and deviation from the sums at its two ends
RV_HD inline void event_stats(double s_en, double q_en, double s_st, double q_st, double len, double* mean, double* stdv) {
  const double m = (s_en - s_st) / len;
  double v = (q_en - q_st) / len - m * m;
  *mean = m;
  *stdv = sqrt(fmax(v, kFltMin));
}

}  // namespace evcore
