// What an entry point calls around its launch, defined in csrc/runtime.hip (internal: not part of include/simpb_hip.h).
#pragma once

extern "C" int simpb_check_launch(void);                            // SIMPB_OK, or SIMPB_ELAUNCH with the text kept for simpb_last_error()
extern "C" int simpb_timing_begin(int kernel_id, void* stream);     // returns a slot, or -1 when timing is off or full
extern "C" void simpb_timing_end(int slot, void* stream);
