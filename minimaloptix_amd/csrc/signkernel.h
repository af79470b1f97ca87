// signkernel.h -- launch interface of signkernel.hip (the signed point queries' table of pseudonormals, pt_sign.h)
#pragma once
#include <hip/hip_runtime.h>
#include "pt_sign.h"

namespace pt {

// The table build: everything device memory.  The topology's arrays (pt_signtopo.h) are uploaded once; facePos is the device copy of the
// faces the refit reads, nine floats per original face id.
struct SignBuildArgs {
  int nFaces, nVerts, nEdges;
  const float* facePos;
  const int* faceIds;                                  // six per face
  const int* vertexStart; const int* vertexCorner;     // nVerts + 1; corners
  const int* edgeStart; const int* edgeFace;           // nEdges + 1; faces
  SignFace* faces;                                     // scratch: nFaces
  v4* vertexN; v4* edgeN;                              // scratch: nVerts, nEdges
  SignRecord* table;                                   // out: nFaces
};
// Three passes on `stream`: per face (unit normal, corner angles), per welded vertex and per edge (the ordered sums), per face (the record).
hipError_t launch_sign_table(hipStream_t stream, const SignBuildArgs& a);

}  // namespace pt
