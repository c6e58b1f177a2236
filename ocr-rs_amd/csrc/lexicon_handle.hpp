// The lexicon handle behind an ocr_lexicon_t*: created and destroyed in lexicon.hip, read by the match calls of lexicon.hip and
// lexicon_lattice.hip.
#pragma once
#include "api_internal.hpp"
#include "lexicon_host.hpp"

struct ocr_lexicon {
  int device = 0;
  ocr::LexPacked host;   // start[] and n are read by every match; the arrays are released after the upload
  void* dev = nullptr;   // codes | lens | index, carved
  size_t o_codes = 0, o_lens = 0, o_index = 0;
  ~ocr_lexicon() {
    if (dev) {
      (void)hipSetDevice(device);
      (void)hipDeviceSynchronize();   // whatever was queued with the lexicon has finished before its memory goes
      (void)hipFree(dev);
    }
  }
};
