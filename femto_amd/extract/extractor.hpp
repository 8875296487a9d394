// extractor.hpp -- what an open extractor holds (extract.hip makes and frees it): the handle it works on, the path it takes and
// the tables in HBM.  lines.hip (../lines/) reads the text through it: ix->d_txt, the dense -> alpha table and doc_ends.
// Included after ../csrc/api_internal.hpp.
#pragma once
#include <cstdint>
#include <memory>
#include <mutex>
#include <vector>

// device buffers a module keeps with the extractor between its calls (hamming.hip, leven.hip); `delete` of the extractor releases them
struct ExtractorWork {
  virtual ~ExtractorWork() = default;
};

struct femto_amd_extractor {
  femto_amd_index* ix = nullptr;    // the handle the work runs on (replica 0 of a multi-device handle)
  bool multi = false;               // opened on a multi-device handle: host forms only
  int path = 0;                     // FEMTO_AMD_EXTRACT_PATH_TEXT / _SAMPLES
  int shift = 0;                    // s: one sample every 2^s positions
  int samp32 = 1;                   // 4-byte sample entries
  int64_t bytes = 0;                // the one allocation below (counted against the handle's budget)
  double build_ms = 0;
  void* block = nullptr;            // [alpha u16 x 256][doc_ends i64 x ndocs][eof rows i64 x ndocs][samples]
  uint16_t* d_alpha = nullptr;      // dense code of d_txt -> alpha code (text path)
  int64_t* d_doc_ends = nullptr;
  int64_t* d_eof = nullptr;
  void* d_samp = nullptr;
  std::vector<int64_t> h_eof;
  std::mutex work_mu;                       // guards the making of `hamming` and `leven`
  std::unique_ptr<ExtractorWork> hamming;   // ../hamming/hamming.hip: its work area, made on first use
  std::unique_ptr<ExtractorWork> leven;     // ../leven/leven.hip: likewise
};
