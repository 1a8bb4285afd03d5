// segment.h -- what segment.hip shares with the rest of the library: stocs_trim (ingest.hip) gives the calling thread's cached
// segmentation workspace, pinned block and clock events back through this.
#ifndef STOCS_SEGMENT_H
#define STOCS_SEGMENT_H
namespace stocs {
void segment_trim();   // nothing of the thread's last stocs_segment_frame is in flight (the call synchronises before it returns)
}
#endif
