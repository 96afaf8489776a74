/* Dense live mode ("Dense live mode"): a window every k <= 8 frames, a `now` stream with no look-ahead, and
 * every frame the mean of all windows that cover it.  Included from gem_hip.h (which declares gem_handle and gem_live_buffers); the
 * three functions are exported by the same library.
 *
 * At stride k window w covers the frames [k w, k w + 10).  A dense session keeps the rings and the state block of gem_live_buffers
 * (gem_live_push is unchanged) and a second block of the caller's, GEM_LIVE_DENSE_DOUBLES doubles, zeroed once:
 *     0       t_prev of the filter over the `now` stream      1  1 once that filter has seen a frame
 *     2       windows emitted      3  frames settled      4  `now` frames written      5..15  unused
 *     16..31  how many windows have been added to each of the GEM_LIVE_DENSE_SLOTS slots (frame n lives in slot n mod 16)
 *     32..79  x_prev [48]      80..127  dx_prev [48]      (the filter's state per coordinate)
 *     128..895   the slots' sums over their covering windows so far [16][48]
 *     896..1663  the slots' estimated frames [16][48]
 * Nothing is allocated, copied to the host or synchronised.
 *
 * gem_live_window_at: gem_live_window for the frames [first_frame, first_frame + 10) (the same kernel; gem_live_window is this call
 * with first_frame = 8 window).  A window that is not complete (n_pushed < first_frame + 10) or whose first frame has been
 * overwritten (n_pushed - first_frame > GEM_LIVE_RING) is refused with a status and gem_last_error; nothing is launched.
 *
 * gem_live_emit_dense: d_global [10,J,3] f64 is the result of window `window` at stride `stride` (1 .. 8).  One launch
 *   - adds the window's 10 frames to their slots (the first window to reach a slot is stored as it is);
 *   - writes the `now` frames to d_out[2]: all 10 of window 0, else the window's last `stride` frames, unaveraged; with h_one_euro
 *     (host, 3 doubles, or NULL: off) they pass the One-Euro filter of gem_one_euro in frame order with the frames' own timestamps;
 *   - writes the `stride` frames [stride w, stride w + stride), which no later window covers, to d_out[0] as sum / count in f64 -- the
 *     covering windows summed oldest first, ((G_a + G_b) + ...) / count, never filtered -- and their estimated frames cams . pose
 *     (the expression of gem_live_emit) to d_out[1]; clears those slots.
 * At stride 8 d_out[0] and d_out[1] carry the bits of gem_live_emit.  final != 0: the 10 - stride frames still held,
 * [stride window, stride window + 10 - stride) with `window` the number of windows emitted, each divided by its own count, to
 * d_out[0] and their estimated frames to d_out[1]; d_global, d_win_pose and d_win_cams are not read, no `now` frame is written and
 * the filter's state stays.  d_out is [3][10][J*3] f64: settled, estimated, now; rows beyond the counts above are left alone.
 *
 * gem_merge_dense: the same mean for recorded windows, at any stride 1 .. T.  d_windows [n_chunks*windows_per_chunk, T, n_coords] f64
 * -> d_out [n_chunks, (windows_per_chunk - 1)*stride + T, n_coords] f64; one thread per (frame, coordinate) sums the covering windows
 * of its chunk in ascending order and divides by their number.  No scratch memory, no read-back: the bytes do not depend on the
 * call or on the chunks that share it.  stride = T - overlap with 2 overlap <= T gives the bits of gem_merge_windows without
 * smoothing. */
#ifndef GEM_LIVE_DENSE_H
#define GEM_LIVE_DENSE_H

#define GEM_LIVE_DENSE_SLOTS 16
#define GEM_LIVE_DENSE_DOUBLES 1664
int gem_live_window_at(gem_handle* h, const gem_live_buffers* b, int64_t first_frame, int64_t n_pushed, const float* d_bone_fixed,
                       float* d_win_pose, double* d_win_cams, float* d_win_heat, float* d_mean_bone, void* stream);
int gem_live_emit_dense(gem_handle* h, const gem_live_buffers* b, double* d_dense_state, int stride, int64_t window, int final,
                        const double* d_global, const float* d_win_pose, const double* d_win_cams, const double* h_one_euro, double* d_out,
                        void* stream);
int gem_merge_dense(const double* d_windows, int n_chunks, int windows_per_chunk, int T, int n_coords, int stride, double* d_out,
                    void* stream);

#endif
