// The f64 float rules: DeviceDecoder::run_group<double> and every kernel it launches.
#include "run_group.hip.h"

namespace ldpc {
template int DeviceDecoder::run_group<double>(Workspace &, const GroupCall &);
}  // namespace ldpc
