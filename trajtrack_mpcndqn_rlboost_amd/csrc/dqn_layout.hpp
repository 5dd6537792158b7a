// dqn_layout.hpp -- the parameter vector of the ray Q-network as include/mpcgpu_dqn.h lays it out (QNetwork.parameters() in
// order: W0 [HID][OBS], b0, W1 [HID][HID], b1, W2 [ACT][HID], b2), the ONLY derivation of its offsets on the device.  Used by
// the update (dqngpu.hip) and by the action rule of the collection kernel (dqn_act.hpp); their forward passes are their own.
#pragma once

#include "../../include/mpcgpu_dqn.h"

namespace dqn_layout {

constexpr int OBS = MPCGPU_DQN_OBS, HID = MPCGPU_DQN_HIDDEN, ACT = MPCGPU_DQN_ACTIONS, NP = MPCGPU_DQN_PARAMS;
constexpr int OFF_W0 = 0, OFF_B0 = OFF_W0 + HID * OBS, OFF_W1 = OFF_B0 + HID, OFF_B1 = OFF_W1 + HID * HID,
              OFF_W2 = OFF_B1 + HID, OFF_B2 = OFF_W2 + ACT * HID;
static_assert(OFF_B2 + ACT == NP, "parameter layout of mpcgpu_dqn.h");

}  // namespace dqn_layout
