// Host side of the message transfer between band levels and pyramid scales (carry.hip; the
// definition: include/stereo_hip.h): the argument checks of stereo_band_carry / stereo_band_carry_device.  No device
// call here or in carry_host.cpp, so that both link into a stand-alone host program (tools/sanitize_carry.cpp).
#pragma once
#include <cstddef>
#include <cstdint>

namespace stereo {
namespace carry {

constexpr int kMaxOldLabels = 4096;   // what a TRW-S plan takes (stereo_trws_plan_path 5)
constexpr int kMaxNewLabels = 512;    // band_common.h: kMaxOffsets (stereo_band_max_offsets)

struct Args {
  const double *M_old = nullptr;
  int64_t E_old = 0;
  int K_old = 0;
  const double *off_old = nullptr;         // host
  const int32_t *edge_src = nullptr;       // may be NULL
  const int32_t *receiver_new = nullptr;
  int64_t N_new = 0;
  const double *shift = nullptr;
  double stretch = 1.0, gain = 1.0;
  const double *off_new = nullptr;         // host
  int K_new = 0;
  int64_t E_new = 0;
  double *M_new = nullptr;
  const void *bad = nullptr;               // may be NULL
  // the device copies of the two offset vectors (the device form alone)
  bool device_form = false;
  const double *d_off_old = nullptr, *d_off_new = nullptr;
};

// 0, or nonzero with the reason (`what`: the entry's name; the message names the argument) in err
int check_args(const char *what, const Args &a, char *err, size_t errcap);

}  // namespace carry
}  // namespace stereo
