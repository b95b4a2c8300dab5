// Host-side streaming event detector: two-window t-statistic peak detector
// restated from /root/reference/event_detection/event_detector.py:75-210 (EventDetector.run,
// _add_sample, _compute_tstat, _detect_peak, _create_event), itself Scrappie-derived.  The
// reference is a pure-Python per-sample loop (~1e5 samples/s); this is the same arithmetic in
// C++ (float64 ring buffer of running sums, uint32 wrap of the sample clock as in to_u32 :281-283).
// Pinned against the reference's own output: tests/golden/events_*.npz, tests/test_events.py.
#include "../../include/ravvent_hip.h"
#include "event_core.h"

#include <cstdint>
#include <vector>

// The arithmetic itself -- t-statistic, peak step, event statistics, the wrapped indices -- is event_core.h's, shared with the device
// kernels of signal_prep.hip; here: the ring buffer of running sums and the per-sample loop around it.

extern "C" int rv_detect_events(const double* raw, size_t n, int32_t w1, int32_t w2, double threshold1,
                                double threshold2, double peak_height, int64_t* start, int64_t* length,
                                double* mean, double* stdv, size_t capacity, size_t* n_events) {
  if (!raw || !n_events || w1 < 1 || w2 < 1 || w2 < w1) return RV_EINVAL;
  using namespace evcore;
  const int buf_len = 1 + 2 * w2;
  std::vector<double> sum(buf_len, 0.), sumsq(buf_len, 0.);
  uint32_t t = 1;
  int64_t evt_st = 0; double evt_st_sum = 0., evt_st_sumsq = 0.;
  Detector sd = make_detector(threshold1, w1), ld = make_detector(threshold2, w2);
  // is_short follows the reference's test `detector['window_length'] == short_detector['window_length']`
  // (:168), which is also true for the long detector when both windows are equal.
  const bool long_is_short = w1 == w2;
  auto ts = [&](uint32_t buf_mid, int w) {
    if (tstat_is_zero(t, w)) return 0.;
    const TstatSlots k = tstat_slots(buf_mid, w, buf_len);
    return tstat(sum[k.st], sumsq[k.st], sum[k.i], sumsq[k.i], sum[k.en], sumsq[k.en], w);
  };
  size_t cnt = 0;
  for (size_t k = 0; k < n; ++k) {                              // _add_sample :85-107
    const double x = raw[k];
    const uint32_t tm = t % buf_len;
    const uint32_t prev = tm > 0 ? tm - 1 : buf_len - 1;
    sum[tm] = sum[prev] + x;
    sumsq[tm] = sumsq[prev] + x * x;
    t += 1;
    const uint32_t buf_mid = buf_mid_of(t, buf_len);
    const double t1 = ts(buf_mid, w1), t2 = ts(buf_mid, w2);
    const bool p1 = detect_peak(t1, sd, ld, true, buf_mid, peak_height);
    const bool p2 = detect_peak(t2, ld, ld, long_is_short, buf_mid, peak_height);
    if (p1 || p2) {                                             // _create_event :189-210
      const uint32_t evt_en = evt_en_of(buf_mid, w1);
      const uint32_t eb = evt_en % buf_len;
      const double len = event_len(evt_en, evt_st);
      if (len < kFltMin) continue;
      double m, v;
      event_stats(sum[eb], sumsq[eb], evt_st_sum, evt_st_sumsq, len, &m, &v);
      if (cnt < capacity && start && length && mean && stdv) {
        start[cnt] = evt_st; length[cnt] = (int64_t)len; mean[cnt] = m; stdv[cnt] = v;
      }
      ++cnt;
      evt_st = evt_en; evt_st_sum = sum[eb]; evt_st_sumsq = sumsq[eb];
    }
  }
  *n_events = cnt;
  return cnt > capacity && start ? RV_EINVAL : RV_OK;
}
