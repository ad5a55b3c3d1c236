// scenegraph_host.h — a tbvh_scenegraph_desc validated and compiled into the flat arrays of scenegraph.h's SgView (scenegraph_host.cpp): what the host
// twin runs on as it is and what capi_scenegraph.hip uploads.  Host only.
#pragma once
#include <vector>

#include "../../include/tinybvh_amd.h"
#include "scenegraph.h"

namespace tbvh {

struct SgCompiled {
    uint32_t nNodes = 0, nSamplers = 0, nChannels = 0, nInstances = 0, nPairs = 0, nAnimations = 0, nUses = 0;
    std::vector<uint32_t> sInterp, sType, sKeyOff, sValOff;
    std::vector<float> times, values;
    std::vector<uint32_t> cSampler, cNode, cTarget, cFlags, cTrig, animOff;   // animOff: nAnimations + 1 entries into the channels
    std::vector<float> cT;
    std::vector<int32_t> cK;
    std::vector<uint32_t> wOff, written;
    std::vector<float> trs, weights, matrix, local, combined, combinedPrev;   // (both combined arrays start as identities)
    std::vector<uint32_t> ancOff, anc;
    std::vector<uint32_t> walkOrder;   // the nodes in visit order (a parent before its children)
    std::vector<int32_t> parent;
    std::vector<uint32_t> instNode;
    std::vector<uint32_t> useOff, pairMesh, pairJoint, pairStale;             // useOff: nUses + 1 entries into the pairs
    std::vector<float> invBind;
    float maxTime = 0;   // 65536 * the shortest non-zero sampler duration (infinity without one): |dt| and |t| beyond it are refused
};

// validates desc (who: the entry point's name for the message) and fills out; 0 or the error code (tbvh_last_error() set)
int sg_compile(const tbvh_scenegraph_desc* desc, const char* who, SgCompiled& out);
// the refusal of a time Channel::Update's wrap loop would not digest; NaN passes (the loops then do nothing, as in the reference)
int sg_check_time(const SgCompiled& g, const char* who, float v);
// bytes and source array of tbvh_scenegraph_download( what ) given the graph's counts; 0 bytes for an unknown `what`
uint64_t sg_download_bytes(const SgCompiled& g, int what);

}  // namespace tbvh
