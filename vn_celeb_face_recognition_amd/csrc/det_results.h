// The result path shared by the detectors (mtcnn_host.cpp, retina.hip): both leave `fin`, rows of 15 floats
// [x1,y1,x2,y2,score, 10 landmark coordinates] at `row_stride` rows per frame, and `fin_cnt`, the rows of every frame.
#pragma once
#include <string>

#include "engine.h"

namespace vnf {

// vnf_*_detect, first half: per-frame counts -> counts / *n_out and the max_out rule (VNF_E_CAPACITY when they exceed it);
// *maxf = rows of the fullest frame, 0 when there is nothing to deliver
int count_results(const char* who, const int* cnt, int b, int32_t* counts, int max_out, int32_t* n_out, int* maxf);
// second half: host rows (b, maxf, 15) -> boxes / probs / points, frames concatenated in order
void scatter_rows(const float* rows, int maxf, const int* cnt, int b, float* boxes, float* probs, float* points);

// vnf_*_results_device: device-resident copy of the last detection (last_b frames; 0: it found nothing)
int results_device(const char* who, const float* fin, const int* fin_cnt, int last_b, int row_stride, int32_t* frame_idx,
                   float* boxes, float* probs, float* points, int max_out, void* stream);

}  // namespace vnf
