// kb.h — what the key-blocked attention kernels share (attn_kb.hip: softmax(q k^T) v at head widths 24 / 48 / 96; attn_relpos_kb.hip: the
// relative-position attention of NBC on long sequences): the geometry of the 64-row LDS blocks of a head's rows.  The images themselves (row stride
// DH + 16 bytes), their staging and their fragments are attn_tiles.h's.
#pragma once
#include "launch.h"

#define KB_THREADS 256
#define KB_BLK 64        // rows per LDS block = rows per workgroup (4 waves x one 16-row tile)
#define KB_TMAX 256      // frames per sequence of the training entry points (forward + backward)
#define KB_TLONG 4096    // frames per sequence of the forward-only *_long_fwd entry points
