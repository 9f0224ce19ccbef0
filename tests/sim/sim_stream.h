// TEST INFRASTRUCTURE -- the stream behind a sim_create handle (sim_lib.cpp), for the doors that work on such handles.
#ifndef AECM_TESTS_SIM_STREAM_H_
#define AECM_TESTS_SIM_STREAM_H_

#include <stdint.h>

#include <vector>

#include "aecm_host_state.h"

struct SimStream {
    aecm::StreamImage img;
    std::vector<uint16_t> hist;
    SimStream() : hist(aecm::kHistWordsPerStream, 0) {}
};

#endif  // AECM_TESTS_SIM_STREAM_H_
