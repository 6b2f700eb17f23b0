// lep_handles.h -- what the C ABI's lep_jpeg / lep_file handles hold (lep_api.cc makes and fills them; lep_stream.cc reads a lep_file).
#pragma once
#include <string>

#include "jpeg_model.h"
#include "lep_container.h"

struct lep_gpu;
namespace lep {
// the text lep_gpu_last_error returns, set by a whole-file call that refuses a file before it reaches a device entry point; returns code
int gpu_refuse(lep_gpu* g, int code, const std::string& what);
}

struct lep_jpeg {
    lep::JpegFile jf;
    lep::EncodeOptions opt;
};
struct lep_file {
    lep::LepFile lf;
    bool frame_ready = false;
    lep::RecodePlan plan;
    bool planned = false;
    lep::ProgPlan prog;
    bool prog_planned = false;
};
