// Pose windows on the device: what pose_windows.hip offers the other host units.
#pragma once
#include <hip/hip_runtime.h>

namespace mi355 {

constexpr int PW_WAVES = 4;            // windows per workgroup: one wave each
constexpr int PW_MAX_TV = 768;         // seq_len * V a window may have (its x and y planes live in LDS)

// every refusal of mi355_pose_windows / mi355_shopformer_score_poses, on the host, before any device call; 0 or MI355_EINVAL
int pose_windows_validate(const void* poses, int dtype, int P, int V_src, const int* starts, int n, int seq_len, int V, int neck);

// one launch for n > 0 windows on device pointers; *launches is incremented beside the launch; nullptr or the HIP error string
const char* launch_pose_windows(const void* poses_dev, int dtype, int V_src, const int* starts_dev, int n, int seq_len, int V, int neck,
                                float* windows_dev, hipStream_t stream, long long* launches);

}  // namespace mi355
