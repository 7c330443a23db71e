// Written by gen_tsdf_tables.py -- do not edit.  Marching tetrahedra over the six Kuhn tetrahedra of a cube.
#pragma once
struct TsdfCase { int n; int e[6]; };            // n triangles; e[3 * t + k] = i * 4 + j: the tetrahedron edge (i, j), i < j
struct TsdfTet { int c[4][3]; int odd; };        // corner offsets (dx, dy, dz); odd: swap v1 and v2 of every triangle
static __constant__ const TsdfCase kTsdfCases[16] = {
  {0, { 0,  0,  0,  0,  0,  0}},   // case  0
  {1, { 1,  2,  3,  0,  0,  0}},   // case  1
  {1, { 1,  7,  6,  0,  0,  0}},   // case  2
  {2, { 2,  3,  7,  2,  7,  6}},   // case  3
  {1, { 2,  6, 11,  0,  0,  0}},   // case  4
  {2, { 1, 11,  3,  1,  6, 11}},   // case  5
  {2, { 1,  7, 11,  1, 11,  2}},   // case  6
  {1, { 3,  7, 11,  0,  0,  0}},   // case  7
  {1, { 3, 11,  7,  0,  0,  0}},   // case  8
  {2, { 1,  2, 11,  1, 11,  7}},   // case  9
  {2, { 1, 11,  6,  1,  3, 11}},   // case 10
  {1, { 2, 11,  6,  0,  0,  0}},   // case 11
  {2, { 2,  6,  7,  2,  7,  3}},   // case 12
  {1, { 1,  6,  7,  0,  0,  0}},   // case 13
  {1, { 1,  3,  2,  0,  0,  0}},   // case 14
  {0, { 0,  0,  0,  0,  0,  0}},   // case 15
};
static __constant__ const TsdfTet kTsdfTets[6] = {
  {{{0, 0, 0}, {1, 0, 0}, {1, 1, 0}, {1, 1, 1}}, 0},   // axes (0, 1, 2)
  {{{0, 0, 0}, {1, 0, 0}, {1, 0, 1}, {1, 1, 1}}, 1},   // axes (0, 2, 1)
  {{{0, 0, 0}, {0, 1, 0}, {1, 1, 0}, {1, 1, 1}}, 1},   // axes (1, 0, 2)
  {{{0, 0, 0}, {0, 1, 0}, {0, 1, 1}, {1, 1, 1}}, 0},   // axes (1, 2, 0)
  {{{0, 0, 0}, {0, 0, 1}, {1, 0, 1}, {1, 1, 1}}, 0},   // axes (2, 0, 1)
  {{{0, 0, 0}, {0, 0, 1}, {0, 1, 1}, {1, 1, 1}}, 1},   // axes (2, 1, 0)
};
