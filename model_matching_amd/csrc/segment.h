// segment.h -- what segment.hip shares with the rest of the library: stocs_trim (ingest.hip) trims its own thread cache and gives the
// calling thread's segmentation cache (thread_cache.h: arenas and pinned block) and the clock's events back through this.
#ifndef STOCS_SEGMENT_H
#define STOCS_SEGMENT_H
namespace stocs {
void segment_trim();   // nothing of the thread's last stocs_segment_frame is in flight (the call synchronises before it returns)
void segment_shapes_trim();   // segment_shapes.hip's cache, the same way (segment_trim calls it: stocs_trim gives both back)
}
#endif
