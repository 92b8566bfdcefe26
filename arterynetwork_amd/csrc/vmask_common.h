// vmask_common.h - what the translation units behind include/vmask.h share: the error text of vmask_last_error,
// the host / device pointer test and the argument check (defined in vmask_device.hip).
#pragma once
#include <cstdint>
#include <string>

namespace vmask {

void set_error(const std::string& msg);
bool is_device_pointer(const void* p);
// the shape test of check_args alone, for a call with a second volume: no device is looked for, no error text set
bool shape_in_envelope(int64_t n0, int64_t n1, int64_t n2);
// shape inside the 32-bit envelope, a usable device (made current): VRG_OK or VRG_E_ARG / VRG_E_NOGPU, error text set
int check_args(int device, int64_t n0, int64_t n1, int64_t n2);

}  // namespace vmask
