// The workspace layouts of the data layer.  Every workspace is laid out by ONE function on a Carver (data_prims.h): on a
// measuring Carver it gives the size (xxx_workspace), on the real base it fills the launch's pointers (xxx_carve); either way it returns
// the bytes handed out.  Included by the files that define them (points.hip, text.hip, polygon.hip, overlay.hip, surface.hip) and by
// tools/workspace_layout_check.cpp, which is why they are declared at all.
#pragma once
#include "data_prims.h"
#include "kernels.h"

size_t blockmedian_layout(BlockMedianLaunch& a, long n, long hw, Carver c);
size_t text_structure_layout(TextLaunch& a, size_t nbytes, Carver c);
size_t text_parse_layout(TextLaunch& a, size_t ncand, int nuse, Carver c);
size_t polygon_layout(PolyLaunch& a, bool stage_edges_too, double** staged, Carver c);
size_t overlay_layout(OverlayLaunch& a, bool stage_prims_too, double** staged, Carver c);
struct SurfaceArrays {   // the solver's state, two partial sums per workgroup, four float64 planes, the free-node mask
  void* state;
  double *part, *x, *r, *p, *ap;
  unsigned char* mask;
};
size_t surface_layout(SurfaceArrays& v, long H, long W, Carver c);
