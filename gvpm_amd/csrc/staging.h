// The staging ring (context.h: StagingRing) as gvpm_gather sees it.  uploads.hip holds its one implementation: the producer
// side behind gvpm_upload_* / gvpm_prefetch_*, and these two ends of a gather.
#pragma once
#include "context.h"

// Head of a gather: the compute streams wait for the copies of the current slots; packed inputs are decoded on `us`, the
// stream at the head of the chain that reads them (G-BRE builds on the build stream), and `other` waits for the decode.
int stagingHead(gvpm_context *h, hipStream_t us, hipStream_t other);
// Tail: the kernels just queued are the last readers of the current slots; prefetched slots become the current ones.
int stagingTail(gvpm_context *h);
