// gs_splat_file.h -- what a gs_splat_file handle holds: gs_splat_file_open (gs_import.cpp) fills it, gs_import_file_to_asset (gs_bake.hip) reads it.
// Host only, no HIP.
#pragma once
#include <cstdio>
#include <vector>

#include "../../include/gsplat_c.h"

struct gs_splat_file {
    gs_splat_file_info info = {};
    FILE* f = nullptr;              // PLY: the open file; the vertex rows start at bodyAt
    long long bodyAt = 0;
    std::vector<uint8_t> raw;       // SPZ: the gunzipped stream, info.body_bytes of it checked
    ~gs_splat_file() { if (f) fclose(f); }
};

namespace gs {
bool splat_file_is_open(const gs_splat_file* file);      // a handle gs_splat_file_open returned and gs_splat_file_close has not yet seen
}
