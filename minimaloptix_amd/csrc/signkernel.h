// signkernel.h -- launch interface of signkernel.hip (signed point queries and their table of pseudonormals, pt_sign.h)
#pragma once
#include <hip/hip_runtime.h>
#include "pointkernel.h"
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

struct PointSignedArgs {
  PointArgs p;                    // out: n x PointHit
  const SignRecord* table;        // one record per original face id; may be null in a scene without triangles
};
// The point kernel's launch (launch_pointquery) with the signed epilogue; the stack overflow area is the point queries' own.
hipError_t launch_pointsigned(hipStream_t stream, const PointSignedArgs& a, int nBlocks);

}  // namespace pt
