// The f32 float rules: DeviceDecoder::run_group<float> and every kernel it launches.
#include "run_group.hip.h"

namespace ldpc {
template int DeviceDecoder::run_group<float>(Workspace &, const GroupCall &);
}  // namespace ldpc
