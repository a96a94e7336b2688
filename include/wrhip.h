/* wrhip.h -- C ABI of libwrhip, the MI355X (gfx950) draw backend for WebRender.
 *
 * Drop-in boundary: these are exactly the 99 `extern "C"` functions that
 * WebRender's software-GL shim binds in the reference
 * (swgl/src/swgl_fns.rs:23-322 of servo/webrender @ 2024-12-20, cited per
 * function below as "fns:<line>"), with the same names, argument meaning and
 * error behaviour (sticky GL error read by GetError, only GL_OUT_OF_MEMORY is
 * ever raised -- swgl/src/gl.cc:1125-1134).  `impl Gl for Context`
 * (swgl_fns.rs:500-2489) links against these unchanged; see INTEGRATION.md.
 *
 * Plain C types only: no torch / HIP types cross this boundary.  All pointers
 * are host pointers.  Calls are made from one thread after MakeCurrent().
 * Rendering is deferred and executed by HIP kernels on the context's stream;
 * Finish(), ReadPixels(), GetColorBuffer(flush=1) and MapBuffer-style host
 * reads synchronise as the GL contract requires.
 */
#ifndef WRHIP_H
#define WRHIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef int8_t GLbyte;
typedef uint8_t GLubyte;
typedef int16_t GLshort;
typedef uint16_t GLushort;
typedef int32_t GLint;
typedef uint32_t GLuint;
typedef int64_t GLint64;
typedef uint64_t GLuint64;
typedef float GLfloat;
typedef double GLdouble;
typedef uint32_t GLenum;
typedef uint8_t GLboolean;
typedef uint32_t GLbitfield;
typedef int32_t GLsizei;
typedef size_t GLsizeiptr;
typedef intptr_t GLintptr;
typedef void GLvoid;
typedef char GLchar;

/* Opaque handles (swgl_fns.rs:17-20, gl.cc:747). */
typedef struct WrhipContext WrhipContext;
typedef struct LockedTexture LockedTexture;

/* YuvRangedColorSpace, composite.h (passed through to CompositeYUV). */
typedef int32_t YuvRangedColorSpace;

/* ---- state ------------------------------------------------------------ */
void ActiveTexture(GLenum texture);                                 /* fns:24  gl.cc:1376 */
void BindTexture(GLenum target, GLuint texture);                    /* fns:25  gl.cc:1590 */
void BindBuffer(GLenum target, GLuint buffer);                      /* fns:26  gl.cc:1594 */
void BindVertexArray(GLuint vao);                                   /* fns:27  gl.cc:1583 */
void BindFramebuffer(GLenum target, GLuint fb);                     /* fns:28  gl.cc:1598 */
void BindRenderbuffer(GLenum target, GLuint rb);                    /* fns:29  gl.cc:1608 */
void BlendFunc(GLenum srgb, GLenum drgb, GLenum sa, GLenum da);     /* fns:30  gl.cc:1325 */
void BlendColor(GLfloat r, GLfloat g, GLfloat b, GLfloat a);        /* fns:31  gl.cc:1336 */
void BlendEquation(GLenum mode);                                    /* fns:32  gl.cc:1341 */
void Enable(GLenum cap);                                            /* fns:33  gl.cc:1097 */
void Disable(GLenum cap);                                           /* fns:34  gl.cc:1111 */
/* ---- queries ---------------------------------------------------------- */
void GenQueries(GLsizei n, GLuint* result);                         /* fns:35  gl.cc:1383 */
void BeginQuery(GLenum target, GLuint id);                          /* fns:36  gl.cc:1540 */
void EndQuery(GLenum target);                                       /* fns:37  gl.cc:1556 */
void GetQueryObjectui64v(GLuint id, GLenum pname, GLuint64* params);/* fns:38  gl.cc:1571 */
/* ---- object creation -------------------------------------------------- */
void GenBuffers(int32_t n, GLuint* result);                         /* fns:39  gl.cc:1397 */
void GenTextures(int32_t n, GLuint* result);                        /* fns:40  gl.cc:1858 */
void GenFramebuffers(int32_t n, GLuint* result);                    /* fns:41  gl.cc:1896 */
void GenRenderbuffers(int32_t n, GLuint* result);                   /* fns:42  gl.cc:1873 */
/* ---- buffers ---------------------------------------------------------- */
void BufferData(GLenum target, GLsizeiptr size, const GLvoid* data,
                GLenum usage);                                      /* fns:43  gl.cc:2007 */
void BufferSubData(GLenum target, GLintptr offset, GLsizeiptr size,
                   const GLvoid* data);                             /* fns:44  gl.cc:2021 */
void* MapBuffer(GLenum target, GLbitfield access);                  /* fns:45  gl.cc:2030 */
void* MapBufferRange(GLenum target, GLintptr offset, GLsizeiptr length,
                     GLbitfield access);                            /* fns:46  gl.cc:2035 */
GLboolean UnmapBuffer(GLenum target);                               /* fns:52  gl.cc:2044 */
/* ---- textures / framebuffers ----------------------------------------- */
void TexStorage2D(GLenum target, GLint levels, GLenum internal_format,
                  GLsizei width, GLsizei height);                   /* fns:53  gl.cc:1732 */
void FramebufferTexture2D(GLenum target, GLenum attachment, GLenum textarget,
                          GLuint texture, GLint level);             /* fns:60  gl.cc:2070 */
GLenum CheckFramebufferStatus(GLenum target);                       /* fns:67  gl.cc:2362 */
void InvalidateFramebuffer(GLenum target, GLsizei num_attachments,
                           const GLenum* attachments);              /* fns:68  gl.cc:2534 */
void TexImage2D(GLenum target, GLint level, GLint internal_format,
                GLsizei width, GLsizei height, GLint border, GLenum format,
                GLenum ty, const void* data);                       /* fns:69  gl.cc:1818 */
void TexSubImage2D(GLenum target, GLint level, GLint xoffset, GLint yoffset,
                   GLsizei width, GLsizei height, GLenum format, GLenum ty,
                   const void* data);                               /* fns:80  gl.cc:1791 */
void GenerateMipmap(GLenum target);                                 /* fns:91  gl.cc:1830 */
/* ---- programs / vertex arrays ----------------------------------------- */
GLint GetUniformLocation(GLuint program, const GLchar* name);       /* fns:92  gl.cc:1507 */
void BindAttribLocation(GLuint program, GLuint index,
                        const GLchar* name);                        /* fns:93  gl.cc:1489 */
GLint GetAttribLocation(GLuint program, const GLchar* name);        /* fns:94  gl.cc:1498 */
void GenVertexArrays(int32_t n, GLuint* result);                    /* fns:95  gl.cc:1412 */
void VertexAttribPointer(GLuint index, GLint size, GLenum type_,
                         GLboolean normalized, GLsizei stride,
                         const GLvoid* offset);                     /* fns:96  gl.cc:1929 */
void VertexAttribIPointer(GLuint index, GLint size, GLenum type_,
                          GLsizei stride, const GLvoid* offset);    /* fns:104 gl.cc:1949 */
GLuint CreateShader(GLenum shader_type);                            /* fns:111 gl.cc:1425 */
void AttachShader(GLuint program, GLuint shader);                   /* fns:112 gl.cc:1439 */
GLuint CreateProgram(void);                                         /* fns:113 gl.cc:1455 */
void Uniform1i(GLint location, GLint v0);                           /* fns:114 gl.cc:2049 */
void Uniform4fv(GLint location, GLsizei count, const GLfloat* value);/* fns:115 gl.cc:2055 */
void UniformMatrix4fv(GLint location, GLsizei count, GLboolean transpose,
                      const GLfloat* value);                        /* fns:116 gl.cc:2061 */
/* ---- the hot path ----------------------------------------------------- */
void DrawElementsInstanced(GLenum mode, GLsizei count, GLenum type_,
                           GLintptr indices, GLsizei instancecount);/* fns:122 gl.cc:2702 */
void EnableVertexAttribArray(GLuint index);                         /* fns:129 gl.cc:1969 */
void VertexAttribDivisor(GLuint index, GLuint divisor);             /* fns:130 gl.cc:1996 */
void LinkProgram(GLuint program);                                   /* fns:131 gl.cc:1471 */
GLint GetLinkStatus(GLuint program);                                /* fns:132 gl.cc:1482 */
void UseProgram(GLuint program);                                    /* fns:133 gl.cc:1082 */
void SetViewport(GLint x, GLint y, GLsizei width, GLsizei height);  /* fns:134 gl.cc:1093 */
void FramebufferRenderbuffer(GLenum target, GLenum attachment,
                             GLenum renderbuffertarget,
                             GLuint renderbuffer);                  /* fns:135 gl.cc:2085 */
void RenderbufferStorage(GLenum target, GLenum internalformat, GLsizei width,
                         GLsizei height);                           /* fns:141 gl.cc:1910 */
void DepthMask(GLboolean flag);                                     /* fns:142 gl.cc:1350 */
void DepthFunc(GLenum func);                                        /* fns:143 gl.cc:1352 */
void SetScissor(GLint x, GLint y, GLsizei width, GLsizei height);   /* fns:144 gl.cc:1363 */
void ClearColor(GLfloat r, GLfloat g, GLfloat b, GLfloat a);        /* fns:145 gl.cc:1367 */
void ClearDepth(GLdouble depth);                                    /* fns:146 gl.cc:1374 */
void Clear(GLbitfield mask);                                        /* fns:147 gl.cc:2498 */
void ClearTexSubImage(GLenum target, GLint level, GLint xoffset, GLint yoffset,
                      GLint zoffset, GLsizei width, GLsizei height,
                      GLsizei depth, GLenum format, GLenum ty,
                      const void* data);                            /* fns:148 gl.cc:2370 */
void ClearTexImage(GLenum target, GLint level, GLenum format, GLenum ty,
                   const void* data);                               /* fns:161 gl.cc:2490 */
void ClearColorRect(GLuint fbo, GLint xoffset, GLint yoffset, GLsizei width,
                    GLsizei height, GLfloat r, GLfloat g, GLfloat b,
                    GLfloat a);                                     /* fns:162 gl.cc:2520 */
void PixelStorei(GLenum name, GLint param);                         /* fns:173 gl.cc:1612 */
void ReadPixels(GLint x, GLint y, GLsizei width, GLsizei height, GLenum format,
                GLenum ty, void* data);                             /* fns:174 gl.cc:2556 */
void Finish(void);                                                  /* fns:183 gl.cc:2802 */
void ShaderSourceByName(GLuint shader, const GLchar* name);         /* fns:184 gl.cc:1431 */
void TexParameteri(GLenum target, GLenum pname, GLint param);       /* fns:185 gl.cc:1854 */
void CopyImageSubData(GLuint src_name, GLenum src_target, GLint src_level,
                      GLint src_x, GLint src_y, GLint src_z, GLuint dst_name,
                      GLenum dst_target, GLint dst_level, GLint dst_x,
                      GLint dst_y, GLint dst_z, GLsizei src_width,
                      GLsizei src_height, GLsizei src_depth);       /* fns:186 gl.cc:2608 */
void CopyTexSubImage2D(GLenum target, GLint level, GLint xoffset, GLint yoffset,
                       GLint x, GLint y, GLsizei width,
                       GLsizei height);                             /* fns:203 gl.cc:2650 */
void BlitFramebuffer(GLint src_x0, GLint src_y0, GLint src_x1, GLint src_y1,
                     GLint dst_x0, GLint dst_y0, GLint dst_x1, GLint dst_y1,
                     GLbitfield mask, GLenum filter);               /* fns:213 composite.h:434 */
void GetIntegerv(GLenum pname, GLint* params);                      /* fns:225 gl.cc:1151 */
void GetBooleanv(GLenum pname, GLboolean* params);                  /* fns:226 gl.cc:1197 */
const char* GetString(GLenum name);                                 /* fns:227 gl.cc:1209 */
const char* GetStringi(GLenum name, GLuint index);                  /* fns:228 gl.cc:1226 */
GLenum GetError(void);                                              /* fns:229 gl.cc:1126 */
/* ---- swgl extensions -------------------------------------------------- */
void InitDefaultFramebuffer(int32_t x, int32_t y, int32_t width, int32_t height,
                            int32_t stride, void* buf);             /* fns:230 gl.cc:2302 */
void* GetColorBuffer(GLuint fbo, GLboolean flush, int32_t* width,
                     int32_t* height, int32_t* stride);             /* fns:238 gl.cc:2322 */
void ResolveFramebuffer(GLuint fbo);                                /* fns:245 gl.cc:2345 */
void SetTextureBuffer(GLuint tex, GLenum internal_format, GLsizei width,
                      GLsizei height, GLsizei stride, void* buf,
                      GLsizei min_width, GLsizei min_height);       /* fns:246 gl.cc:2354 */
void SetTextureParameter(GLuint tex, GLenum pname, GLint param);    /* fns:256 gl.cc:1834 */
void DeleteTexture(GLuint n);                                       /* fns:257 gl.cc:1865 */
void DeleteRenderbuffer(GLuint n);                                  /* fns:258 gl.cc:1890 */
void DeleteFramebuffer(GLuint n);                                   /* fns:259 gl.cc:1903 */
void DeleteBuffer(GLuint n);                                        /* fns:260 gl.cc:1404 */
void DeleteVertexArray(GLuint n);                                   /* fns:261 gl.cc:1419 */
void DeleteQuery(GLuint n);                                         /* fns:262 gl.cc:1390 */
void DeleteShader(GLuint shader);                                   /* fns:263 gl.cc:1451 */
void DeleteProgram(GLuint program);                                 /* fns:264 gl.cc:1460 */
LockedTexture* LockFramebuffer(GLuint fbo);                         /* fns:265 composite.h:485 */
LockedTexture* LockTexture(GLuint tex);                             /* fns:266 composite.h:497 */
void LockResource(LockedTexture* resource);                         /* fns:267 composite.h:510 */
void UnlockResource(LockedTexture* resource);                       /* fns:268 composite.h:518 */
void* GetResourceBuffer(LockedTexture* resource, int32_t* width,
                        int32_t* height, int32_t* stride);          /* fns:269 composite.h:540 */
void Composite(LockedTexture* locked_dst, LockedTexture* locked_src, GLint src_x,
               GLint src_y, GLsizei src_width, GLsizei src_height, GLint dst_x,
               GLint dst_y, GLsizei dst_width, GLsizei dst_height,
               GLboolean opaque, GLboolean flip_x, GLboolean flip_y,
               GLenum filter, GLint clip_x, GLint clip_y, GLsizei clip_width,
               GLsizei clip_height);                                /* fns:275 composite.h:560 */
void CompositeYUV(LockedTexture* locked_dst, LockedTexture* locked_y,
                  LockedTexture* locked_u, LockedTexture* locked_v,
                  YuvRangedColorSpace color_space, GLuint color_depth,
                  GLint src_x, GLint src_y, GLsizei src_width,
                  GLsizei src_height, GLint dst_x, GLint dst_y,
                  GLsizei dst_width, GLsizei dst_height, GLboolean flip_x,
                  GLboolean flip_y, GLint clip_x, GLint clip_y,
                  GLsizei clip_width, GLsizei clip_height);         /* fns:295 composite.h:1330 */
WrhipContext* CreateContext(void);                                  /* fns:317 gl.cc:2816 */
void ReferenceContext(WrhipContext* ctx);                           /* fns:318 gl.cc:2818 */
void DestroyContext(WrhipContext* ctx);                             /* fns:319 gl.cc:2825 */
void MakeCurrent(WrhipContext* ctx);                                /* fns:320 gl.cc:2808 */
size_t ReportMemory(WrhipContext* ctx,
                    size_t (*size_of_op)(const void* ptr));         /* fns:321 gl.cc:2840 */

/* ---- libwrhip additions (not part of the reference ABI) --------------- *
 * Introspection / measurement hooks used by bench.py and the tests.  None of
 * them is needed by the Rust side.                                        */

/* Last-flush statistics: kernel launches, raster-kernel GPU nanoseconds
 * (hipEvent on the context stream), algorithmic bytes of the raster launch. */
typedef struct WrhipStats {
  uint64_t flushes;            /* flush_all() calls that launched work      */
  uint64_t kernel_launches;    /* HIP kernel launches since reset           */
  uint64_t raster_launches;    /* launches of the tile raster kernel        */
  uint64_t raster_ns;          /* summed GPU time of raster launches (events) */
  uint64_t raster_algo_bytes;  /* summed algorithmic bytes      */
  uint64_t raster_pixels;      /* destination pixels owned by those launches */
  uint64_t prims;              /* instances rasterised                      */
  uint64_t h2d_bytes;          /* bytes uploaded host->HBM                  */
  uint64_t d2h_bytes;          /* bytes read back HBM->host                 */
  /* host time spent inside the library (std::chrono, nanoseconds): where the CPU side of a frame goes */
  uint64_t host_record_ns;     /* DrawElementsInstanced: state snapshot + instance bytes             */
  uint64_t host_upload_ns;     /* TexSubImage2D / TexImage2D / BufferData / BufferSubData: staging of uploaded bytes */
  uint64_t host_flush_ns;      /* flush: descriptor arena, staging copy, kernel launches (no waiting) */
  uint64_t host_wait_ns;       /* Finish / ReadPixels / queries: blocked on the stream               */
  uint64_t row_launches;       /* launches of the row kernels (wr_span_rows_kernel / wr_tile_rows_kernel); included in raster_launches */
  uint64_t setup_carried;      /* flushes whose setup stage (and upload scatter) went out in a held-back raster launch of the flush before */
  uint64_t carrier_lost;       /* flushes that planned such a carrier and found the held-back launches already gone (0 unless broken) */
  uint64_t scratch_grown_held; /* scratch buffers of a flush replaced while the launches of the flush before were held back */
  uint64_t forwarded_targets;  /* targets whose finished pixels were also stored through to the target an opaque 1:1 composite copies them to */
  uint64_t cell_bins;          /* bins launched on the rect-only RGBA8 raster variant with the cell raster on: each that starts from a clear
                                  goes through wr_raster_cells (0 in the host simulation, which has no cell raster) */
} WrhipStats;
void WrhipGetStats(WrhipStats* out);
void WrhipResetStats(void);
/* Enable hipEvent timing of every kernel launch (one event pair and a sync per launch: for measurement runs only).
 * 1: every flush launches its own kernels at once (what a Finish per frame gives); 2: the launches stay where throughput
 * mode issues them -- raster launches held back to the next flush, the first of them fused with that flush's setup stage. */
void WrhipSetProfiling(int enabled);
/* Per-kernel-variant totals collected while profiling is on: kind 0 = upload scatter, 1 = setup stage, 3 = mask rows (wr_mask_rows_kernel), 2 = raster
 * kernel wr_raster_kernel<fmt, depth, 4, feat>, 4 = a chained run of thin R8 levels, 5 = wr_raster_dense_kernel, 6 / 7 = kinds 2 / 5
 * fused with the next flush's setup stage (wr_setup_raster[_dense]_kernel: setup bytes and workgroups added), 8 = wr_setup_rows_kernel
 * (3 fused likewise), 9 = wr_span_rows_kernel (the cs_blur / cs_scale targets of a level, a wave per target row piece), 10 = wr_tile_rows_kernel
 * (picture targets of a few large gradient / image prims, likewise), 11 = wr_setup_tile_rows_kernel (10 fused with the next flush's setup stage), 12 = a thin launch of the raster kernel (13: the same with the next flush's setup stage in front, wr_setup_raster_thin_kernel) (wr_raster_kernel<fmt, false, 1, feat>:
 * small levels, several workgroups per bin), 14 = wr_tap_kernel (WrhipTapTexture: fmt of the tapped texture, feat 1 against an expected texture;
 * algo_bytes: the rect's bytes, twice with an expected texture), 15 = wr_grab_pack_kernel (WrhipGrabTexture: fmt of the grabbed texture,
 * feat 1 in delta mode, feat 2: wr_grab_pack_runs_kernel, a WRHIP_GRAB_PACKED delta, feat 3: wr_grab_scale_kernel, the launches of one WrhipGrabTextureScaled, feat 4: wr_grab_tensor_kernel or the launches of a scaled WrhipGrabTextureTensor, feat 5: wr_grab_yuv_kernel, a WrhipGrabTextureYuv (the rect read once plus the planes written), feat 6: wr_grab_yuv_delta_kernel, a WrhipGrabTextureYuvDelta (the rect plus the retained planes; what its sent blocks write is not known at the launch, as for feat 1), feat 7: wr_grab_scale_yuv_kernel, the launches of one WrhipGrabTextureYuvScaled (the rect read once plus the planes of every rendition written), feat 8: wr_grab_scroll_*_kernel, the WRHIP_GRAB_SCROLL_LAUNCHES launches of one scroll grab that is no keyframe as one entry (the rect plus the retained copy, as for feat 2); algo_bytes: bytes read plus bytes written, as far as they are known at the launch), 16 = wr_put_tensor_kernel (WrhipPutTextureTensor: fmt of the texture written;
 * algo_bytes: the elements read plus the rect's bytes written).  algo_bytes: the launch's algorithmic bytes:
 * raster launches count every destination pixel they own once (twice when the target's old content is loaded) plus
 * the source texels their draws can sample; the setup stage counts instance + descriptor + record bytes.  Returns the
 * number of entries written (<= max). */
typedef struct WrhipKernelStat {
  int32_t kind, fmt, depth, feat;
  uint64_t launches, ns, algo_bytes, workgroups;
} WrhipKernelStat;
int32_t WrhipGetKernelStats(WrhipKernelStat* out, int32_t max);
/* Restrict rasterisation to tile-rows owned by `rank` of `world` (multi-GPU
 * sharding by render-target strips). world<=1 disables. */
void WrhipSetShard(int rank, int world);
/* Restrict rasterisation of render target `tex` to pixel rows [y0,y1) (rows
 * outside are neither computed nor stored); y0==y1 removes the restriction;
 * y1<y0, or a range outside the texture, means the target is not this
 * process's at all: draws and clears into it are dropped when recorded (no
 * instance snapshot, staging, upload or setup work).  Used by the multi-GPU
 * harness to give each rank a screen-space strip. */
void WrhipSetTargetRows(GLuint tex, int32_t y0, int32_t y1);
/* Device pointer + geometry of a texture's HBM storage (for RCCL gather). */
void* WrhipGetTextureDevicePtr(GLuint tex, int32_t* width, int32_t* height,
                               int32_t* stride);
/* Texture id of an FBO's colour attachment (fbo 0 = default framebuffer). */
GLuint WrhipGetFramebufferTexture(GLuint fbo);
/* Width and height of a texture's storage as recorded so far: a state query that submits nothing and waits for nothing
 * (returns 0, leaving the outputs alone, for an unknown texture or one without storage). */
int32_t WrhipGetTextureSize(GLuint tex, int32_t* width, int32_t* height);
/* Name of the HIP device the context runs on, or NULL if none. */
const char* WrhipDeviceName(void);
/* Submit everything recorded so far to the context's HIP stream (pending draws, queued uploads, the
 * held-back composite level) WITHOUT waiting for it: after the call the stream holds all the work
 * whose results a consumer enqueued behind it on the same stream will see.  The multi-GPU harness
 * orders its framebuffer-strip copy and the RCCL all-gather this way instead of a Finish per frame. */
void WrhipFlush(void);
/* ... the same, leaving this flush's own raster launches held back for the next flush (returns 1 if they are): see wrhip.hip */
int WrhipFlushHeld(void);
/* The context's hipStream_t (NULL in the host simulation), e.g. for torch.cuda.ExternalStream. */
void* WrhipGetStream(void);
/* Texture taps: a reduction over a texture rect, enqueued on the context's stream behind whatever was issued before it and
 * delivered to the host later -- a reftest harness or a frame loop checks every frame without a ReadPixels, which would stall
 * the pipeline and copy the whole window.
 *
 * WrhipTapTexture(tex, x, y, w, h, expected) reduces the w x h rect at (x, y) of `tex` (GL_RGBA8 or GL_R8; the window is
 * WrhipGetFramebufferTexture(0); rows as stored: row r of the rect is texture row y + r) and returns a ticket >= 0.
 *   digest[j]  the sum over the rect's pixels, mod 2^64, of mix(k_i + C_j): i = r * w + c, k_i = (uint64)i << 32 | v_i, v_i the
 *              pixel's four stored bytes as a little-endian word (its one byte for R8), C_0 = 0x9E3779B97F4A7C15,
 *              C_1 = 0xD1B54A32D192ED03, mix(z): z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9, z = (z ^ z >> 27) * 0x94D049BB133111EB,
 *              z ^ z >> 31.  Exact integer arithmetic: any restatement gives the same 128 bits.
 *   hist[d]    with `expected` != 0 (a texture of the same format holding at least w x h pixels, compared from ITS origin): the
 *              pixels whose largest absolute channel difference is d -- wrench's reftest measure; max_diff and differing are
 *              its two summaries (taken from the bins on the host).  Without `expected` every pixel is in hist[0].
 * The tap sees exactly the draws, clears, uploads, blits and composites issued before the call.  Recorded work is submitted as by
 * WrhipFlushHeld: nothing is waited for, and raster launches that are held back for the next flush stay held back -- a tap of a
 * texture they write is issued directly behind them whenever they leave (the next flush, WrhipFlushHeld, Finish, a readback).
 * Later writes to either texture, deleting it or giving it new storage do not change the result.
 * Returns -1 and sets GL_INVALID_VALUE, launching nothing, for an unknown texture or format, a rect that is empty or not inside
 * `tex`, an `expected` of another format or too small, and while sharding is on (WrhipSetShard world > 1, WrhipSetTargetRows on
 * `tex`).
 *
 * WrhipTapResultGet(ticket, out, wait): 0 and *out filled; 1 if the result has not arrived yet (wait == 0 only; wait != 0 first
 * sends what the tap is parked behind, then waits for this ticket alone, not for the stream); -1 for a ticket that was never
 * handed out or has been overwritten -- the ring holds the 64 newest. */
typedef struct WrhipTapResult {
  int32_t  status;        /* 0 ok */
  uint32_t width, height; /* the rect actually reduced */
  uint32_t format;        /* GL_RGBA8 or GL_R8 */
  uint64_t digest[2];
  uint32_t max_diff;      /* 0 without an expected texture */
  uint32_t differing;     /* pixels with difference > 0 */
  uint32_t hist[256];     /* hist[d] = pixels whose difference is exactly d; all in hist[0] without an expected texture */
} WrhipTapResult;
int32_t WrhipTapTexture(GLuint tex, int32_t x, int32_t y, int32_t w, int32_t h, GLuint expected);
int32_t WrhipTapResultGet(int32_t ticket, WrhipTapResult* out, int32_t wait);
/* Texture grabs: the taps' sibling that delivers the pixels -- whole rects, or only the 64 x 64 blocks of a rect that changed since
 * the previous grab of it -- in stream order, behind held-back launches, through tickets, without a Finish or a ReadPixels.
 *
 * WrhipGrabTexture(tex, rects, nrects, flags) enqueues a grab of `nrects` rects (x, y, w, h each) of `tex` (GL_RGBA8 or GL_R8; the
 * window is WrhipGetFramebufferTexture(0)) and returns a ticket >= 0.  Pixels are the stored bytes (RGBA8 textures hold B, G, R,
 * A); row r of a rect is texture row y + r.
 * Ordering is the taps': the grab sees exactly what was issued before the call; recorded work is submitted as by WrhipFlushHeld;
 * nothing is waited for; raster launches that are held back stay held back, and a grab of a texture they write is issued directly
 * behind them whenever they leave.  Later writes to the texture, new storage for it or deleting it do not change the result.
 * Full mode (no WRHIP_GRAB_DELTA): 1 to 16 rects, each non-empty and inside `tex`; they may overlap.  FLIP_ROWS and SWAP_RB apply
 *   to every rect.  WrhipGrabResultGet copies them to `dst`: one rect as h rows of w * bpp bytes at `dst_stride` (0: tight); several
 *   rects one after another, each tight (`dst_stride` must be 0).
 * Delta mode (WRHIP_GRAB_DELTA): one rect, neither FLIP_ROWS nor SWAP_RB.  The library keeps one retained copy of the rect in HBM
 *   per texture, valid until the texture gets new storage or is deleted, a delta grab names another rect, or WRHIP_GRAB_KEY is
 *   passed.  Blocks are 64 x 64 pixels, aligned to the rect's origin, edge blocks cut to the rect.  A block is sent when any stored
 *   byte of it differs from the retained copy, and every block is sent when there is no valid retained copy (a keyframe); the
 *   same grab brings the retained copy up to date.  In WrhipGrabResultGet `dst` is the caller's own image of the rect (h rows at
 *   `dst_stride`, 0: tight): the sent blocks are patched into it and nothing else is touched.
 * Packed delta mode (WRHIP_GRAB_DELTA | WRHIP_GRAB_PACKED, with or without KEY): a delta grab whose sent blocks are written in the
 *   lossless packed form below.  Retained copy, block comparison and keyframe rules are the plain delta grab's, and plain and packed
 *   delta grabs of one texture and rect may alternate without a keyframe: PACKED changes only how a sent block is written.
 * Returns -1 and sets GL_INVALID_VALUE, launching nothing, for an unknown texture or format, no rects or more than 16, a rect that
 * is empty or not inside `tex`, an unknown flag, DELTA with several rects or with FLIP_ROWS / SWAP_RB, KEY or PACKED without DELTA, SWAP_RB on
 * GL_R8, and while sharding is on (WrhipSetShard world > 1, WrhipSetTargetRows on `tex`).  Returns -1 with GL_OUT_OF_MEMORY when the
 * pinned host memory of the ticket ring would exceed WRHIP_GRAB_PINNED_MAX bytes (environment; default 512 MB): every one of the 8
 * ring entries keeps a device and a pinned slot as large as the largest grab it carried (a delta grab: all blocks of the rect).
 *
 * WrhipGrabResultGet(ticket, info, dst, dst_stride, wait): 0 with *info filled and, unless `dst` is NULL, the pixels delivered; 1 if
 * the result has not arrived yet (wait == 0 only; wait != 0 first sends what the grab is parked behind, then waits for this ticket
 * alone, not for the stream); -1 for a ticket that was never handed out or has been overwritten -- the ring holds the 8 newest --
 * and, with GL_INVALID_VALUE, for a `dst_stride` below a row's bytes or a non-zero one with several rects.  A result may be fetched
 * any number of times while its ticket lives.  `bytes` counts what crossed to the host: WRHIP_GRAB_HEADER bytes and the payload --
 * the rects' bytes in full mode, blocks * (16 + 64 * 64 * bpp) in delta mode (a 16-byte record and the block at a fixed pitch), the
 * sum of the entries' sizes in packed delta mode, where `blocks` counts the entries and `damage` bounds them;
 * WrhipStats::d2h_bytes grows by it when the ticket is first fetched, by this call or by WrhipGrabPayloadGet.  A delta payload that
 * does not parse (status 1) is delivered as far as its entries are good ones: the library's own kernels never write such a one.
 *
 * WrhipGrabPayloadGet(ticket, dst, capacity, bytes, wait): the bytes that crossed, of a grab of any mode, as they lie in the pinned
 * slot -- the 16-byte header (word 0: the payload's bytes), then the payload --, for a consumer that forwards them.  0 with *bytes =
 * header + payload and the first min(capacity, *bytes) of them copied to `dst` (which may be NULL with capacity 0); 1: not arrived
 * (wait == 0 only); -1: a dead ticket.  Parking and `wait` are WrhipGrabResultGet's.
 *
 * WrhipGrabDecode(payload, bytes, format, flags, rect_w, rect_h, dst, dst_stride, damage, blocks): a pure host function -- no
 * context, no GPU -- that patches a delta payload (`payload`: its header; `flags`: the grab's, PACKED or not; `format`: GL_RGBA8 or
 * GL_R8) into the caller's image `dst` of the rect (rows of `dst_stride` bytes, 0: tight; NULL: only checked) and returns 0 with the
 * entries' bounding box and number (either may be NULL), or -1 for a malformed payload, having written nothing.
 * WrhipGrabResultGet decodes through the same code (webrender_amd/csrc/wr_grab_codec.h, which a program can include on its own).
 *
 * THE PACKED PAYLOAD (a contract: one content has one encoding, only the order of the entries is free).
 *   A sequence of entries, each starting on 16 bytes and a multiple of 16 bytes long: a 16-byte record, then a body.  The record is
 *   four little-endian 32-bit words:  0: x of the block, relative to the rect;  1: y likewise;  2: w | h << 8 | mode << 16, w and h
 *   in 1..64 (the block cut to the rect);  3: aux.
 *   The block's pixels in row-major order over the CUT block are p_0 .. p_{w*h-1}; a pixel's value is its 4 stored bytes as a word
 *   (RGBA8) or its byte (R8).  Pixel i starts a run if i = 0 or value(p_i) != value(p_{i-1}) -- the first pixel of a row is compared
 *   with the last pixel of the row above.  n is the number of run starts.
 *     mode 0 RAW    neither of the others applies.  aux 0.  Body: 64 rows at a pitch of 64 * bpp, as in a plain delta entry; the
 *                   bytes beyond the cut block are zero.
 *     mode 1 SOLID  n = 1.  aux: the value (R8: the byte, zero-extended).  No body.
 *     mode 2 RUNS   n > 1 and 16 + align16(8 * h + n * bpp) < 16 + 4096 * bpp.  aux: n.  Body: h words of 64 bits, one per block
 *                   row, bit c set when pixel (r, c) starts a run, bits at c >= w zero; then the n start values in order (n * bpp
 *                   bytes); then zero bytes to the next multiple of 16.
 *   A tie between RUNS and RAW goes to RAW: a full RGBA8 block is RUNS up to n = 3964 and RAW from 3965, a full R8 block RUNS up
 *   to n = 3568 and RAW from 3569.  No entry is larger than a plain delta entry, so slots are sized as for a plain delta grab.
 *
 * THE SCROLL GRAB (WRHIP_GRAB_DELTA | WRHIP_GRAB_PACKED | WRHIP_GRAB_SCROLL, with or without KEY; GL_RGBA8 and GL_R8): a packed delta
 *   grab that first finds the one vertical scroll most of the changed content made, and sends a block that is found that many rows
 *   away in the retained copy as a 16-byte COPY entry: "take it from your own image".  SCROLL in any other combination -- without
 *   DELTA, without PACKED, with FLIP_ROWS / SWAP_RB, on the scaled and tensor calls, on WrhipGrabTextureYuv and
 *   WrhipGrabTextureYuvScaled -- is -1 with GL_INVALID_VALUE, nothing launched.  It uses the plain and packed delta grabs' retained copy under the same validity rules and keeps no other state, so
 *   plain, packed and scroll delta grabs of one texture and rect may alternate in any order without a keyframe.  A keyframe is the
 *   packed grab's (one launch, scroll_dy 0, no COPY entry); any other scroll grab is WRHIP_GRAB_SCROLL_LAUNCHES launches on the draw
 *   stream.  The contract -- any restatement must give the same bytes, up to the order of the entries:
 *   prev is the retained copy, cur the rect's stored bytes, h the rect's height; a segment (r, c) is the bytes of rect row r inside
 *   block column c; D = min(WRHIP_GRAB_SCROLL_MAX, h - 1).
 *   vector    for 1 <= |dy| <= D, votes(dy) = the number of segments (r, c) with 0 <= r + dy < h, cur(r, c) != prev(r, c) and
 *             cur(r, c) == prev(r + dy, c).  scroll_dy is the dy with the most votes; ties go to the smaller |dy|, then to the
 *             positive dy; 0 if no dy has a vote.  Positive: the content moved up, a block's pixels are dy rows further DOWN in the
 *             previous image.  One vector per grab, vertical only.  FOR THE VOTE ONLY the library decides segment equality by a
 *             64-bit hash of the segment's bytes: the rule holds up to hash collisions, which can cost a COPY entry, never a pixel.
 *   blocks    decided by exact byte comparison: a block equal to prev at its own place is not sent; otherwise it is a COPY entry if
 *             scroll_dy != 0, its source rows lie inside the rect (0 <= y + dy, y + dy + block_h <= h) and it equals prev at
 *             (x, y + dy); otherwise SOLID / RUNS / RAW by the packed rule.  The retained copy equals cur after the grab.
 *   wire      header word 1 is scroll_dy as a two's-complement int32 (0 in every other grab's header).  COPY is mode 3: record x, y,
 *             w | h << 8 | 3 << 16, aux 0, no body.  `blocks` counts all entries, `copied` the COPY ones, `damage` bounds all of
 *             them, `bytes` = 16 + the entries' sizes: an unchanged frame crosses 16 bytes, a scrolled one 16 + 16 * copied + the
 *             entries of the exposed strip.
 *   decoding  (WrhipGrabResultGet into the caller's image, WrhipGrabDecode with the grab's flags) is in place, without a snapshot: a
 *             COPY block holds the pixels the image had BEFORE the decode at (x, y + dy), other entries are patched as ever, nothing
 *             else is touched.  All COPY entries are applied first -- by ascending y for dy > 0, descending y for dy < 0; block
 *             columns are independent of each other --, every other entry after them; entries arrive in any order and the decoder
 *             orders them itself.  Malformed, WrhipGrabDecode -1 with nothing written: a COPY entry with dy == 0, |dy| >
 *             WRHIP_GRAB_SCROLL_MAX, a COPY source outside the rect, a COPY record with a non-zero aux, one that is not a whole
 *             block of the rect or names a block twice, mode 3 or a non-zero header word 1 when `flags` lacks SCROLL.
 *   Not supported: horizontal or per-region vectors, COPY of a block whose source is partly outside the rect, sharded targets.
 *   (Scroll detection for delta YUV grabs: WrhipGrabTextureYuvDelta with WRHIP_GRAB_DELTA | WRHIP_GRAB_SCROLL, below.)
 *
 * WrhipGrabTextureScaled(tex, rect, dst_w, dst_h, flags): a grab of ONE rect (x, y, w, h) of a GL_RGBA8 texture scaled down to
 * dst_w x dst_h (1 <= dst_w <= w, 1 <= dst_h <= h), byte for byte what the reference's screenshot chain (webrender's
 * AsyncScreenshotGrabber::scale_screenshot) gets from BlitFramebuffer(.., GL_LINEAR) calls that never halve by more than 2:
 *   levels  L is the smallest L >= 0 with w <= 2 * dst_w * 2^L (the width alone decides); level k is dst_w << k x dst_h << k.
 *   top     BlitFramebuffer(x, y, x + w, y + h, 0, 0, dst_w << L, dst_h << L, COLOR, GL_LINEAR) into level L: linear_blit's 1/128-texel
 *           walk, clamped at the TEXTURE's edges (a tap at the rect's edge reads the texel beyond it where there is one); equal sizes,
 *           or a texture narrower than 2, make it a nearest copy.  The height ratio may be anything.
 *   lower   level k from level k + 1 by BlitFramebuffer(0, 0, dst_w << (k + 1), dst_h << (k + 1), 0, 0, dst_w << k, dst_h << k, COLOR, GL_LINEAR).
 *   result  level 0.
 * One kernel walks the chain tile by tile with the intermediate levels in LDS (a launch per 4 levels beyond the first 4; those hand
 * a level on through HBM).  Ticket ring, ordering, parking behind held-back launches, slot growth, transport, `bytes` and "later
 * writes do not change the result" are a full grab's.  `flags`: FLIP_ROWS and / or SWAP_RB, applied to the delivered rows.  The
 * payload is dst_w * dst_h * 4 bytes; WrhipGrabResultGet delivers dst_h rows of dst_w * 4 bytes at `dst_stride` (0: tight; below
 * dst_w * 4: -1 with GL_INVALID_VALUE) and reports flags | WRHIP_GRAB_SCALED, the rect as given, scaled_w, scaled_h and levels = L.
 * Returns -1 and sets GL_INVALID_VALUE, launching and flushing nothing, for an unknown texture, a format other than GL_RGBA8, a rect
 * that is empty or not inside `tex`, dst_w or dst_h below 1 or above the rect's, dst_w << L or dst_h << L above GL_MAX_TEXTURE_SIZE,
 * any other flag, and while sharding is on; -1 with GL_OUT_OF_MEMORY as WrhipGrabTexture.
 *
 * WrhipGrabTextureTensor(tex, rect, desc): a grab of ONE rect whose pixels never leave the device: they are converted into a tensor
 * of U8, F16, BF16 or F32 elements, planes (CHW) or interleaved (HWC), in the caller's device memory `desc->dst`, and only the
 * ticket's 16-byte header crosses to the host.  The contract -- any restatement must give the same bits:
 *   pixels    out_w x out_h equal to the rect's size: the rect's stored bytes (GL_RGBA8 or GL_R8).  Smaller (GL_RGBA8 only): the bytes
 *             WrhipGrabTextureScaled(tex, rect, out_w, out_h, 0) delivers -- the same level rule, top step and 2:1 steps.
 *   channels  the stored bytes of an RGBA8 pixel are B, G, R, A.  Output channel c takes R, G, B, A in that order, or B, G, R, A with
 *             WRHIP_TENSOR_BGR; channels == 3 drops A.  An R8 texture has the one channel (BGR changes nothing).  With FLIP_ROWS
 *             output row r holds pixel row out_h - 1 - r.
 *   value     U8: the byte v.  Otherwise x = (float)v * scale[c] + bias[c], a float32 multiply and a float32 add, each rounded
 *             once, never fused.  F32 stores x; F16 and BF16 store x rounded to nearest, ties to even: F16 with subnormals (2^-25
 *             and below give zero) and 65520 and above as infinity; a NaN stays a quiet NaN.  (webrender_amd/csrc/wr_tensor_round.h
 *             is the two roundings as integer arithmetic; a program can include it on its own.)
 *   address   element (c, y, x) lies at element index c * plane_stride + y * row_stride + x from `dst` (CHW), or at y * row_stride
 *             + x * channels + c (HWC, plane_stride ignored).  A stride of 0 is the tight one: out_w (CHW) or out_w * channels (HWC)
 *             for a row, out_h * row_stride for a plane.  Nothing but these elements is written: not the padding between rows or
 *             planes, not a byte ahead of `dst` or behind the last element.  `dst` is aligned to the element's size.
 *   ordering  WrhipGrabTexture's: the grab sees exactly what was issued before the call, recorded work is submitted as by
 *             WrhipFlushHeld, nothing is waited for, and a grab of a texture the held-back launches write is parked behind them;
 *             later writes to the texture do not change the result.
 *   ticket    rides the grab ring with an empty payload: its arrival is the completion signal.  WrhipGrabResultGet ignores `dst`
 *             and reports flags | WRHIP_GRAB_TENSOR, the rect, `bytes` = 16, and scaled_w, scaled_h, levels = L of a scaled grab
 *             (all 0 of an unscaled one).  The write does NOT depend on the ticket surviving: a parked tensor grab whose ticket
 *             the ring has overwritten (8 newer grabs) is issued all the same, and only its notification is lost -- other parked
 *             grabs in that position are dropped.
 *   consuming on the device  once a grab has been issued, work enqueued on WrhipGetStream() follows it.  A parked grab is issued by
 *             whatever sends the held-back launches: the next flush, a WrhipFlushHeld() that finds nothing recorded, a waiting
 *             WrhipGrabResultGet, WrhipDeviceFree.  The caller keeps `dst` alive until then.
 * The unscaled grab is one launch (wr_grab_tensor_kernel: 16-byte stores where `dst` and the strides in bytes are multiples of 16,
 * single elements otherwise); a scaled one is the scaled grab's launches, 1 + L / 4, the last of which converts as it stores.
 * Returns -1 and sets GL_INVALID_VALUE, launching and flushing nothing, for: an unknown texture or format; channels other than 3 or
 * 4 (RGBA8) or 1 (R8); a rect that is empty or not inside `tex`; out_w or out_h below 1 or above the rect's; scaling an R8 texture;
 * out_w << L or out_h << L above GL_MAX_TEXTURE_SIZE; an unknown dtype, layout or flag; a NULL desc or dst; a stride below its
 * minimum (CHW: row >= out_w, plane >= (out_h - 1) * row + out_w; HWC: row >= out_w * channels) or above 2^40; an extent in bytes
 * above dst_bytes; a dst not aligned to its element; and while sharding is on.  -1 with GL_OUT_OF_MEMORY as WrhipGrabTexture.
 *
 * WrhipDeviceAlloc(bytes): device memory of this context's runtime, 16-byte aligned (host memory in the host simulation); NULL with
 * GL_OUT_OF_MEMORY when there is none.  bytes == 0 gives a valid allocation of no usable bytes: not NULL, an address of its own,
 * freed like any other.  WrhipDeviceFree(p): first sends what parked grabs wait behind, the grabs with it, then waits for the draw
 * stream, then frees; NULL is ignored.  WrhipDeviceRead(dst_host, src_dev, bytes): a copy on the draw stream behind everything
 * issued so far, waited for; held-back launches stay held -- a parked grab has not written yet: fetch its ticket first.  0, or -1
 * for a NULL pointer.  WrhipStats::d2h_bytes grows by `bytes`.  WrhipDeviceWrite(dst_dev, src_host, bytes): its sibling, host to
 * device on the draw stream behind everything issued so far, waited for; held-back launches stay held.  0, or -1 for a NULL pointer.
 * WrhipStats::h2d_bytes grows by `bytes`.
 *
 * WrhipPutTextureTensor(tex, rect, desc): the way IN, the inverse of a tensor grab: a CHW or HWC tensor of U8, F16, BF16 or F32
 * elements in the caller's device memory `desc->src` is converted on the device into the stored bytes of `rect` of a GL_RGBA8, GL_R8
 * or GL_RG8 texture -- one launch on the draw stream, no pixel crosses to the host.  The contract -- any restatement must give the
 * same bytes:
 *   geometry  the tensor is rect.w x rect.h: no scaling.  With FLIP_ROWS tensor row r goes to rect row h - 1 - r.
 *   address   the tensor grab's: element (c, y, x) lies at element index c * plane_stride + y * row_stride + x from `src` (CHW), or
 *             at y * row_stride + x * channels + c (HWC, plane_stride ignored).  A stride of 0 is the tight one: w (CHW) or
 *             w * channels (HWC) for a row, h * row_stride for a plane.  Nothing but these elements is read -- not the padding
 *             between rows or planes -- and their extent lies inside src_bytes.  `src` is aligned to the element's size.
 *   channels  the stored bytes of an RGBA8 pixel are B, G, R, A.  Input channel c supplies R, G, B, A in that order, or B, G, R, A
 *             with WRHIP_TENSOR_BGR; with channels == 3, A is `desc->alpha`.  An R8 texture takes its one channel; an RG8 texture
 *             takes channel 0 as byte 0 and channel 1 as byte 1 (BGR changes nothing for either).  Values are stored as given: no
 *             premultiplication, no colour conversion.
 *   value     U8: the stored byte is the element; scale and bias are ignored.  Otherwise x is the element widened to float32
 *             exactly (F16 subnormals, infinities and NaNs included; BF16 is a 16-bit shift) and y = x * scale[c] + bias[c] with c
 *             the INPUT channel, a float32 multiply and a float32 add, each rounded once, never fused.  The byte is 0 if y is a NaN
 *             or y < 0, 255 if y >= 255, otherwise y rounded to nearest, ties to even (0.5 -> 0, 1.5 -> 2, 2.5 -> 2) -- the
 *             rounding of swgl's round_pixel on x86.  (webrender_amd/csrc/wr_tensor_round.h holds the two conversions, float16 bits
 *             -> float32 bits and float32 bits -> byte, as integer arithmetic.)
 *   written   exactly the rect's bytes in the texture; no other byte of it is touched.
 *   ordering  a texture write at its place in the call order, like TexSubImage2D or CopyImageSubData: draws recorded before it that
 *             sample or target `tex` see the old bytes (recorded work is flushed), held-back launches that reference `tex` leave
 *             first, queued uploads go out ahead of it; everything recorded, uploaded, tapped or grabbed afterwards sees the new
 *             bytes; a tap or grab issued before it is unchanged.  On a texture that nothing pending touches the put flushes
 *             nothing and leaves held-back launches held.  The read of `src` is enqueued on WrhipGetStream() before the call
 *             returns and is never parked: work the caller enqueued on that stream earlier precedes it, later work follows it; a
 *             caller producing `src` on another stream orders it itself.  One case is handled here: if [src, src + src_bytes)
 *             overlaps the destination of a PARKED tensor grab, what that grab is parked behind is sent first, the grab with it, so
 *             that it has written before the put reads.  Retained copies of delta grabs stay valid (they compare content).
 *   cost      one launch: WrhipStats::kernel_launches grows by 1, h2d_bytes and d2h_bytes by 0.
 * Returns 0; -1 and sets GL_INVALID_VALUE, launching, flushing and changing nothing, for: an unknown texture or one without storage;
 * a format other than GL_RGBA8, GL_R8, GL_RG8; a texture whose storage is a caller's host buffer (SetTextureBuffer) or that is locked;
 * channels other than 3 or 4 (RGBA8), 1 (R8), 2 (RG8); a rect that is empty or not inside `tex`; an unknown dtype, layout or flag;
 * a NULL desc or src; a src not aligned to its element; a stride below the tensor grab's minimum or above 2^40; an extent in bytes
 * above src_bytes; an alpha above 255; and while sharding is on.
 *
 * WrhipPutTexturePayload(tex, rect, payload, bytes, flags): the way IN for delta payloads, the inverse of a delta, packed or scroll
 * grab: the payload is decoded ON THE DEVICE into `rect` of a GL_RGBA8 or GL_R8 texture, at its place in the call order.  Only the
 * payload's bytes (and a small index of its entries) cross to the device; the blocks are expanded there -- WrhipGrabDecode into a
 * host image and TexSubImage2D of the damage rect would carry the uncompressed pixels.  The contract -- any restatement must give
 * the same bytes:
 *   payload   host memory: the 16-byte header, then the entries, as WrhipGrabPayloadGet hands them out; `bytes` is header plus
 *             payload (16 + header word 0).  `flags` are the producing grab's: WRHIP_GRAB_DELTA is required; PACKED, SCROLL (with
 *             PACKED only) and KEY are allowed (KEY changes nothing here); any other flag is an error.  The format is the texture's.
 *             The payload is copied before the call returns: the caller may free it at once.
 *   meaning   after the put, the bytes of `rect` in `tex` are what WrhipGrabDecode(payload, bytes, format, flags, rect.w, rect.h, img,
 *             stride, ..) leaves in `img` when `img` held the rect's bytes before the put.  COPY entries follow the in-place rule:
 *             all are applied first, by ascending y for dy > 0 and descending y for dy < 0, and a COPY block holds what the rect
 *             had BEFORE the put at (x, y + dy); every other entry is applied after them.  Entries may arrive in any order.  Plain
 *             delta entries (record plus block at the fixed pitch), RAW, SOLID, RUNS and COPY are all accepted.
 *   written   exactly the cut blocks the entries name; no other byte of the texture is touched -- not the rest of the rect, not a
 *             byte beyond a cut block.
 *   checked   the whole payload, on the host, with the decoder's own checks (wr_grab_codec.h: wr_gc_entry and the COPY rules)
 *             before anything is launched, staged or flushed: whatever makes WrhipGrabDecode return -1 makes the put return -1.
 *             One payload more is refused: one in which two entries that are no COPY share a pixel.  The host decoder applies
 *             those in payload order; the device gives every entry a workgroup of its own, which has no order.  No grab emits one.
 *   ordering  WrhipPutTextureTensor's: a texture write at its place in the call order.  Draws recorded before it that sample or
 *             target `tex` see the old bytes (recorded work is flushed), held-back launches that reference `tex` leave first, queued
 *             uploads go out ahead of it (the payload travels with their DMA); everything recorded, uploaded, tapped or grabbed
 *             afterwards sees the new bytes; a tap or grab issued before it is unchanged.  On a texture that nothing pending
 *             touches the put flushes no recorded work and leaves held-back launches held.  Retained copies of delta grabs stay
 *             valid (they compare content): a delta grab of `tex` after a put sends the blocks whose bytes the put changed.
 *   cost      WrhipStats::kernel_launches grows by 1 (wr_put_patch_kernel), or by WRHIP_PUT_PAYLOAD_LAUNCHES when the payload has a
 *             COPY entry (wr_put_copy_kernel first; by 1 again if it has nothing else); by 0 for a payload with no entry, which
 *             orders and stages nothing.  h2d_bytes grows by what is staged: `bytes` plus the index, 4 bytes per entry and 4 per
 *             block column with a COPY entry plus 4 -- never more than 16 per entry.  d2h_bytes grows by 0.  Nothing is waited for.
 * Returns 0; -1 and sets GL_INVALID_VALUE, launching, staging, flushing and changing nothing, for: a malformed payload (above); an
 * unknown texture or one without storage; a format other than GL_RGBA8, GL_R8; a texture whose storage is a caller's host buffer
 * (SetTextureBuffer) or that is locked; a rect that is empty or not inside `tex`; a NULL payload; `bytes` below 16 or not 16 plus
 * header word 0; a missing DELTA, SCROLL without PACKED or any other flag; and while sharding is on.  Not supported: YUV delta
 * payloads, payloads in device memory, GL_RG8.
 *
 * WrhipGrabTextureYuv(tex, rect, desc): a grab of ONE rect of a GL_RGBA8 texture as 8-bit Y'CbCr planes for a video encoder -- the
 * inverse of the video that CompositeYUV and brush_yuv_image draw.  One launch (wr_grab_yuv_kernel) converts the rect; the planes
 * cross to the host as the ticket's payload (desc->dst == NULL: 1.5 bytes per pixel in 4:2:0 against a full grab's 4), or are
 * written into the caller's device memory.  The contract -- any restatement must give the same bytes:
 *   pixels    the rect's stored bytes B, G, R, A; A is ignored.  Stored colours are premultiplied, so what is converted is the page
 *             over BLACK; nothing is un-premultiplied.  No scaling.  With FLIP_ROWS image row r is rect row h - 1 - r; the flip
 *             comes first, chroma blocks are formed on the flipped image.
 *   planes    Y is w x h.  WRHIP_YUV_I420: a Cb and a Cr plane of cw x ch samples, cw = (w + 1) / 2, ch = (h + 1) / 2.
 *             WRHIP_YUV_NV12: one plane of ch rows of cw (Cb, Cr) byte pairs.  WRHIP_YUV_I444: a Cb and a Cr plane of w x h.
 *   luma      Y = (Yr * R + Yg * G + Yb * B + (y0 << 16) + 0x8000) >> 16 with y0 = 16 in the narrow ranges and 0 in the full ones;
 *             it cannot leave 0 .. 255.
 *   chroma    I444, per pixel: C = clamp((Cr_ * R + Cg * G + Cb_ * B + (128 << 16) + 0x8000) >> 16, 0, 255).  4:2:0, sample (i, j):
 *             S is the channel-wise sum of the four pixels at image positions (min(2i + dx, w - 1), min(2j + dy, h - 1)), dx, dy in
 *             {0, 1} -- clamped to the RECT, not the texture -- and C = clamp((c . S + (128 << 18) + (1 << 17)) >> 18, 0, 255).
 *             32-bit integer arithmetic, arithmetic right shifts; no intermediate reaches 2^27.  The clamp is live: pure blue or
 *             pure red gives 256 in a full range.
 *   rows      desc->color_space is a YuvRangedColorSpace, 0 .. 5; the rows, R, G, B, in 16.16 fixed point:
 *               0 Rec601Narrow   Y 16829 33039 6416   Cb  -9714 -19070 28784   Cr 28784 -24103 -4681
 *               1 Rec601Full     Y 19595 38470 7471   Cb -11058 -21710 32768   Cr 32768 -27439 -5329
 *               2 Rec709Narrow   Y 11966 40254 4064   Cb  -6596 -22188 28784   Cr 28784 -26145 -2639
 *               3 Rec709Full     Y 13933 46871 4732   Cb  -7509 -25259 32768   Cr 32768 -29763 -3005
 *               4 Rec2020Narrow  Y 14786 38160 3338   Cb  -8038 -20746 28784   Cr 28784 -26469 -2315
 *               5 Rec2020Full    Y 17216 44434 3886   Cb  -9151 -23617 32768   Cr 32768 -30133 -2635
 *             From Kr, Kb = (0.299, 0.114), (0.2126, 0.0722), (0.2627, 0.0593): the real row, times 219 / 255 (Y) or 224 / 255
 *             (chroma) in a narrow range, times 65536, each entry rounded to nearest; then the GREEN entry is adjusted so that a Y
 *             row sums to 56284 (narrow) or 65536 (full) and a chroma row to 0.  So a grey g gives Y = y0 + round(g * 219 / 255)
 *             (or g) and chroma exactly 128, a flat 2 x 2 block gives I444's chroma, and no sample is further than 1 from the
 *             real formula rounded half up.
 *   host sink (dst == NULL; the strides and dst_bytes must be 0)  the payload is the planes, each tight, one after another: Y, Cb,
 *             Cr -- NV12: Y, then the plane of pairs.  It rides the grab ring as a full grab's does: slot growth,
 *             WRHIP_GRAB_PINNED_MAX, transport on the grab stream.  WrhipGrabResultGet copies the payload to `dst` (dst_stride must
 *             be 0: -1 with GL_INVALID_VALUE otherwise) and reports flags | WRHIP_GRAB_YUV, format GL_RGBA8, the rect, `bytes` =
 *             header + payload.  WrhipGrabPayloadGet works as for any grab.
 *   device sink (dst != NULL)  Y row r lies at dst + r * y_stride; the chroma planes follow at dst + h * y_stride, rows c_stride
 *             apart, the second plane of I420 and I444 a further rows * c_stride on.  Strides are in BYTES; 0 is the tight one (w;
 *             cw, 2 * cw for NV12, or w).  Nothing but the planes' samples is written: not the padding of a row, not a byte ahead
 *             of `dst` or behind the last sample.  The ticket carries an empty payload and its arrival is the completion signal
 *             (`bytes` = 16, WrhipGrabResultGet ignores `dst`); the write does NOT depend on the ticket surviving, as for a tensor
 *             grab, and "consuming on the device" is the tensor grab's.  A parked YUV grab's destination takes part in
 *             WrhipPutTextureTensor's overlap rule as a parked tensor grab's does.
 *   ordering  WrhipGrabTexture's, parking and "later writes do not change the result" included.
 *   cost      one launch: WrhipStats::kernel_launches grows by 1, flushes by 0.
 * Returns -1 and sets GL_INVALID_VALUE, launching and flushing nothing, for: an unknown texture or a format other than GL_RGBA8; a
 * rect that is empty or not inside `tex`; an unknown format, colour space (GbrIdentity and above) or flag; a NULL desc; a host sink
 * with a non-zero stride or dst_bytes; a device sink with a stride below its row's bytes or above 2^40, or an extent above
 * dst_bytes; and while sharding is on.  -1 with GL_OUT_OF_MEMORY as WrhipGrabTexture.
 *
 * WrhipGrabTextureYuvDelta(tex, rect, desc, flags): WrhipGrabTextureYuv for a page that is mostly still: only the 64 x 64 blocks
 * whose SAMPLES changed since the previous such grab cross the link (or are written to the caller's planes), with a damage rect
 * for the encoder's skip decisions.  `desc` is WrhipGrabTextureYuv's -- formats, the six colour spaces, FLIP_ROWS, host or device
 * sink --; `flags` is 0, WRHIP_GRAB_KEY and / or WRHIP_GRAB_DELTA | WRHIP_GRAB_SCROLL (`scroll` below).  One launch (wr_grab_yuv_delta_kernel).  The
 * contract -- any restatement must give the same bytes:
 *   samples   exactly those WrhipGrabTextureYuv produces for the same rect and desc: table, luma, chroma, the clamp, 4:2:0 blocks
 *             clamped to the RECT, the flip ahead of the chroma blocks.
 *   blocks    64 x 64 luma samples of the IMAGE (after the flip), aligned to the image's origin, edge blocks cut to the image.  A cut
 *             block of bw x bh has (bw + 1) / 2 x (bh + 1) / 2 chroma samples in 4:2:0 ((bw + 1) / 2 pairs a row for NV12) and
 *             bw x bh in I444.  64 is even: a 2 x 2 chroma block never straddles two blocks, a pixel changes samples of its own
 *             block only.
 *   retained  the library keeps one retained copy of the image's PLANES per texture (pool memory, about 1.5 or 3 bytes per pixel),
 *             apart from the plain delta grab's retained pixels: plain or packed delta grabs and delta YUV grabs of one texture never
 *             invalidate each other.  It is valid until the texture gets new storage or is deleted, a delta YUV grab names another
 *             rect, format, colour space, flip, sink (`dst`) or stride, or KEY is passed.
 *   sent      a block is sent when any sample of its planes differs from the retained planes, and every block when there is no
 *             valid retained copy (a keyframe); the same grab brings the retained copy up to date.  A change of alpha alone never
 *             sends a block, nor does a colour change that rounds to the same samples.
 *   host sink (dst == NULL)  the payload is a sequence of entries of one size: a 16-byte record -- four little-endian 32-bit words
 *             x, y, w, h of the luma block, relative to the image -- and the block's planes at fixed pitches: Y, 64 rows at 64;
 *             then I420: Cb, then Cr, 32 rows at 32 each (an entry: 16 + 6144 bytes); NV12: 32 rows of pairs at 64 (16 + 6144);
 *             I444: Cb, then Cr, 64 rows at 64 each (16 + 12288).  Bytes beyond the cut block are unspecified; no decoder reads
 *             them.  On a keyframe entry i is block i (row-major); otherwise the order of the entries is free.
 *             WrhipGrabResultGet(ticket, info, dst, 0, wait): `dst` is the caller's own tight planes in WrhipGrabTextureYuv's
 *             payload layout (Y, Cb, Cr; NV12: Y, pairs); the sent blocks are patched in and nothing else is touched; a non-zero
 *             dst_stride: -1 with GL_INVALID_VALUE.  info: flags = WRHIP_GRAB_YUV | WRHIP_GRAB_DELTA | desc->flags (| KEY if given),
 *             format GL_RGBA8, keyframe, blocks, blocks_total and damage as a plain delta grab's, `bytes` = 16 + blocks * entry
 *             size.  WrhipGrabPayloadGet works as for any grab.
 *   device sink (dst != NULL)  the sent blocks' samples are written straight into the caller's planes, WrhipGrabTextureYuv's layout
 *             and stride rules; nothing but the samples of sent blocks is written.  The payload is the records alone, 16 bytes per
 *             sent block -- the host still learns blocks and damage --, `bytes` = 16 + 16 * blocks, and WrhipGrabResultGet ignores
 *             `dst`.  The write does NOT depend on the ticket surviving: a parked grab whose ticket was overwritten still patches the
 *             planes and the retained copy; only the records are lost.  The destination takes part in WrhipPutTextureTensor's
 *             overlap rule as a parked YUV grab's does.
 *   ordering, parking, ring, slot growth, WRHIP_GRAB_PINNED_MAX  WrhipGrabTexture's; slots are sized for all blocks of the rect.  A
 *             parked HOST-sink grab that lost its ticket is dropped, and the next delta YUV grab of that texture is a keyframe.
 *   cost      one launch: WrhipStats::kernel_launches grows by 1, flushes by 0.
 *   scroll    (`flags` with WRHIP_GRAB_DELTA | WRHIP_GRAB_SCROLL, beside KEY or not: the flag is spelt with DELTA, as on
 *             WrhipGrabTexture, and either of the two bits without the other stays refused)  a scrolled page changes every block, but nearly all of its samples
 *             sit in the consumer's planes a few rows away: the grab finds the one vertical scroll and sends such blocks as 16-byte
 *             COPY entries.  Without the flag every byte, launch and info field is as described above.  The contract -- any
 *             restatement must give the same bytes, up to the order of the entries: prev is the retained planes, cur the samples
 *             WrhipGrabTextureYuv would produce now for the same rect and desc, both in image space (after FLIP_ROWS); h is the
 *             image's height, a segment (r, c) the LUMA samples of image row r inside block column c, D = min(WRHIP_GRAB_SCROLL_MAX,
 *             h - 1).
 *     candidates  1 <= |dy| <= D; in I420 and NV12 only EVEN dy -- an odd shift moves luma rows across chroma rows and no chroma
 *             sample survives it --, in I444 every dy.
 *     vector  votes(dy) = the number of segments with 0 <= r + dy < h, cur_Y(r, c) != prev_Y(r, c) and cur_Y(r, c) == prev_Y(r + dy,
 *             c).  scroll_dy is the candidate with the most votes; ties go to the smaller |dy|, then to the positive dy; 0 if no
 *             candidate has a vote.  Positive: the content moved up.  FOR THE VOTE ONLY segment equality is decided by a 64-bit hash.
 *     blocks  by exact comparison of samples.  A block is not sent if ALL its samples, Y and chroma, equal prev at its own place.
 *             Otherwise it is a COPY entry if scroll_dy != 0, 0 <= y + dy and y + dy + bh <= h, every Y sample equals prev_Y dy rows
 *             away and every chroma sample equals prev's chroma dy / 2 rows away in 4:2:0, dy rows away in I444; otherwise a
 *             SAMPLES entry.  After the grab the retained planes equal cur.
 *     keyframe  (no valid retained copy, or KEY)  scroll_dy 0, no COPY entry, one launch.  The retained copy is the delta YUV grab's
 *             own, under the same validity rules: delta YUV grabs with and without SCROLL may alternate on one texture, rect and
 *             desc in any order without a keyframe.  (A texture that is grabbed with SCROLL holds a second set of planes of the
 *             same size; the two exchange roles with every such grab.)
 *     wire    (host sink)  header word 1 is scroll_dy as an int32.  EVERY record of a SCROLL grab is x, y, w | h << 8 | mode << 16,
 *             0 -- the packed payload's record layout.  Mode 0, SAMPLES: the record, then the planes exactly as a delta YUV entry
 *             lays them out (16 + 6144 or 16 + 12288 bytes).  Mode 3, COPY: the record alone.  On a keyframe entry i is still block
 *             i.  `bytes` = 16 + the sum of the entries' sizes, `blocks` counts all entries, `copied` the COPY ones, `damage`
 *             bounds all of them, info.flags carries WRHIP_GRAB_SCROLL; slots are sized as without the flag.
 *     device sink  SAMPLES blocks are written into the caller's planes as without the flag.  A COPY block's samples are written
 *             into the caller's planes FROM THE LIBRARY'S retained planes at the shifted place -- never from the caller's planes:
 *             there is no in-place hazard, and it does not matter what the caller did to them.  The payload is the records alone,
 *             16 bytes per entry with the mode word.  Nothing but samples of sent and copied blocks is written, and the write does
 *             not depend on the ticket surviving.
 *     decoding  WrhipGrabResultGet decodes into the caller's host planes; WrhipGrabDecodeYuv decodes with `format |
 *             WRHIP_GRAB_SCROLL` as its format.  In place, without a snapshot: all COPY entries first -- by ascending y for dy > 0,
 *             descending y for dy < 0, on all planes, chroma moved by dy / 2 rows in 4:2:0 --, then all SAMPLES entries.  Malformed,
 *             WrhipGrabDecodeYuv -1 with nothing written: a mode other than 0 or 3; a non-zero word 3; a header word 1 beyond
 *             WRHIP_GRAB_SCROLL_MAX; COPY with dy == 0 or an odd dy in a 4:2:0 format; a COPY source outside the image; an entry
 *             that is not a whole block of the image; a block named twice; mode 3 or a non-zero header word 1 when the SCROLL bit
 *             is absent.
 *     cost    a scroll grab that is no keyframe is WRHIP_GRAB_YUV_SCROLL_LAUNCHES launches on the draw stream (probe, the scroll
 *             grab's vote, pack; no update launch: the probe writes the second set of planes) and 0 flushes.
 *     Not supported: horizontal or per-region vectors, luma-only copies for odd scrolls in 4:2:0, scroll for scaled YUV grabs,
 *             sharded targets.
 * Returns -1 and sets GL_INVALID_VALUE, launching and flushing nothing and leaving the retained copy as it was, for everything
 * WrhipGrabTextureYuv rejects, for any `flags` bit other than KEY, DELTA and SCROLL, and for DELTA without SCROLL or SCROLL
 * without DELTA; -1 with GL_OUT_OF_MEMORY as WrhipGrabTexture.
 *
 * WrhipGrabTextureYuvScaled(tex, rect, out_w, out_h, descs, renditions): a grab of ONE rect of a GL_RGBA8 texture scaled down as
 * WrhipGrabTextureScaled scales it and delivered as WrhipGrabTextureYuv's planes -- at up to four sizes, the lowest levels of the
 * one chain, from a single pass over the source (wr_grab_scale_yuv_kernel: the levels of a tile's pyramid are converted while they
 * are in LDS).  A page rendered at 3840 x 2160 leaves as the 1080p / 540p / 270p ladder of an adaptive stream for the cost of one
 * scaled grab.  The contract -- any restatement must give the same bytes:
 *   chain     WrhipGrabTextureScaled's level rule, unchanged: L is the smallest L >= 0 with rect_w <= 2 * out_w * 2^L, level k is
 *             out_w << k x out_h << k, the top step is a GL_LINEAR BlitFramebuffer of the rect to level L (equal sizes: the nearest
 *             copy), every lower step an exact 2:1 linear blit.
 *   renditions  `renditions` is n, 1 <= n <= min(L + 1, 4).  Rendition k (0 <= k < n) is LEVEL k of that chain -- the definition is the
 *             level, not "a second grab of that size".  Where WrhipGrabTextureScaled(tex, rect, out_w << k, out_h << k, 0) is itself
 *             legal it delivers the same pixels: its L' is L - k and its top level the same.
 *   samples   the level's pixels are treated exactly as WrhipGrabTextureYuv treats a rect of that size: stored B, G, R; A ignored;
 *             FLIP_ROWS first, on the LEVEL's rows; 4:2:0 blocks formed on the flipped image and clamped to the level's last column
 *             and row; the six rows, y0, rounding and the live clamp as there.
 *   descs     descs[k] describes rendition k.  format, color_space and flags must be equal in all of them, and all sinks are the
 *             host or all are the device.
 *   host sink (dst == NULL; the strides and dst_bytes must be 0)  the payload is rendition 0's planes, then rendition 1's, and so on,
 *             each laid out as a WrhipGrabTextureYuv payload of that size: tight, Y then chroma.  WrhipGrabResultGet copies the
 *             payload to `dst` (dst_stride must be 0); slots are sized for the sum.
 *   device sink (dst != NULL)  WrhipGrabTextureYuv's device layout and stride rules, per rendition; nothing but samples is written.
 *             The renditions' extents must not overlap one another.  The ticket carries an empty payload (`bytes` = 16); the write
 *             does NOT depend on the ticket surviving.  Every destination takes part in WrhipPutTextureTensor's overlap rule while
 *             the grab is parked.
 *   ticket    WrhipGrabResultGet reports flags | WRHIP_GRAB_YUV | WRHIP_GRAB_SCALED, format GL_RGBA8, the rect as given, scaled_w /
 *             scaled_h = rendition 0's size, levels = L and renditions = n.  The other grab calls keep rejecting these flags.
 *   ordering, parking, ring, slot growth, WRHIP_GRAB_PINNED_MAX  WrhipGrabTexture's, "later writes do not change the result" included.
 *   cost      WrhipStats::kernel_launches grows by 1 + L / 4 (WrhipGrabTextureScaled's launches: each level is held in LDS by exactly
 *             one of them, and rendition k leaves from the launch that holds level k), flushes by 0.  ONE launch more in a single
 *             case: FLIP_ROWS with a 4:2:0 format and an ODD out_h.  The flipped rendition 0 then pairs level rows (e, e - 1), e
 *             even, which straddle the tiles; the chain leaves level 0 in device scratch and wr_grab_yuv_kernel converts it from
 *             there.  The other renditions of that grab still leave from the chain's launches.
 * Returns -1 and sets GL_INVALID_VALUE, launching and flushing nothing, for everything WrhipGrabTextureScaled rejects for tex, rect,
 * out_w and out_h; everything WrhipGrabTextureYuv rejects for a desc, per rendition, with that rendition's size; `renditions` outside
 * 1 .. min(L + 1, 4); a NULL descs; descs that disagree in format, colour space, flags or sink kind; overlapping device extents; and
 * while sharding is on.  -1 with GL_OUT_OF_MEMORY as WrhipGrabTexture.  out_w x out_h equal to the rect's size with renditions == 1
 * is legal: L = 0 with the nearest copy, WrhipGrabTextureYuv's bytes.
 *
 * WrhipGrabDecodeYuv(payload, bytes, format, rect_w, rect_h, y, y_stride, c0, c1, c_stride, damage, blocks): the pure host function
 * -- no context, no GPU -- behind the host sink's decode (webrender_amd/csrc/wr_grab_codec.h, which a program can include on its
 * own).  It patches a host-sink payload (`payload`: its header) into planes given by pointers and BYTE strides (0: tight); NV12: c0
 * is the plane of pairs and c1 NULL; y, c0 and c1 all NULL: only checked.  0 with the entries' bounding box and number (either may
 * be NULL); -1, having written nothing, for a malformed payload -- a length that is not header + k entries or more than `bytes`
 * holds, an x or y that is no multiple of 64 or outside the image, a w or h that is not the cut block's, more entries than the
 * image has blocks, a non-zero header word 1 -- or for planes given in part or with a stride below a row.  `format |
 * WRHIP_GRAB_SCROLL`: the payload of a SCROLL grab (above), with its own list of what is malformed.
 * Not routed through grabs: Finish, GetColorBuffer, ReadPixels.  Not supported: other formats, sharded targets; scaling other than
 * WrhipGrabTextureScaled's; delta or packed tensor grabs; gamma or colour-space conversion of tensors (values are the stored
 * premultiplied bytes); puts that scale or filter, into other formats, into sharded targets or host-backed textures; YUV grabs of 10-
 * or 16-bit samples (P010), 4:2:2 or YUY2, scaled YUV grabs that scale up, whose renditions are not levels of one chain or differ in format, scaled or packed delta YUV grabs, several rects in one, R8 sources, un-premultiplying, GbrIdentity. */
#define WRHIP_GRAB_FLIP_ROWS 1u   /* full mode: deliver the rect's last row first */
#define WRHIP_GRAB_SWAP_RB   2u   /* full mode, RGBA8 only: bytes 0 and 2 of every pixel exchanged */
#define WRHIP_GRAB_DELTA     4u   /* only the 64x64 blocks that differ from the previous DELTA grab of this texture and rect */
#define WRHIP_GRAB_KEY       8u   /* with DELTA: ignore the retained copy, send every block */
#define WRHIP_GRAB_PACKED    32u  /* with DELTA: sent blocks as SOLID / RUNS / RAW entries (the packed payload above); 16 is no flag */
#define WRHIP_GRAB_SCALED    64u  /* reported in WrhipGrabInfo::flags by a WrhipGrabTextureScaled ticket; no flag of WrhipGrabTexture, which rejects it */
#define WRHIP_GRAB_TENSOR    128u /* reported in WrhipGrabInfo::flags by a WrhipGrabTextureTensor ticket; no flag of the other grab calls, which reject it */
#define WRHIP_GRAB_YUV       512u /* reported in WrhipGrabInfo::flags by a WrhipGrabTextureYuv, (with DELTA) WrhipGrabTextureYuvDelta or (with SCALED) WrhipGrabTextureYuvScaled ticket; rejected by the other grab calls */
#define WRHIP_GRAB_SCROLL    1024u /* with DELTA | PACKED (with or without KEY): find the vertical scroll, send scrolled blocks as COPY entries (the scroll grab above); with DELTA a flag of WrhipGrabTextureYuvDelta too, and a bit of WrhipGrabDecodeYuv's format; rejected in every other combination and by the other grab calls */
#define WRHIP_GRAB_SCROLL_MAX 512      /* the largest |scroll_dy| that is looked for */
#define WRHIP_GRAB_SCROLL_LAUNCHES 4   /* launches on the draw stream of a scroll grab that is no keyframe: probe, vote, pack, update */
#define WRHIP_GRAB_YUV_SCROLL_LAUNCHES 3 /* launches on the draw stream of a delta YUV grab with SCROLL that is no keyframe: probe, vote, pack */
#define WRHIP_YUV_I420 0u         /* WrhipYuvDesc::format: Y plane, Cb plane, Cr plane; chroma 4:2:0 */
#define WRHIP_YUV_NV12 1u         /* Y plane, one plane of interleaved Cb,Cr pairs; chroma 4:2:0 */
#define WRHIP_YUV_I444 2u         /* Y, Cb, Cr planes, all w x h */
#define WRHIP_TENSOR_U8   0u      /* WrhipTensorDesc::dtype */
#define WRHIP_TENSOR_F16  1u
#define WRHIP_TENSOR_BF16 2u
#define WRHIP_TENSOR_F32  3u
#define WRHIP_TENSOR_CHW  0u      /* WrhipTensorDesc::layout: planes */
#define WRHIP_TENSOR_HWC  1u      /* interleaved */
#define WRHIP_TENSOR_BGR  256u    /* WrhipTensorDesc::flags: keep the stored channel order B, G, R(, A); default is R, G, B(, A) */
#define WRHIP_GRAB_MAX_RECTS 16
#define WRHIP_GRAB_HEADER    16u  /* bytes that cross with every grab ahead of its payload (the payload's byte count) */
typedef struct WrhipGrabInfo {
  int32_t  status;                 /* 0 ok */
  uint32_t format, flags;          /* GL_RGBA8 or GL_R8; flags as given */
  int32_t  nrects, rects[WRHIP_GRAB_MAX_RECTS][4];   /* x, y, w, h as given */
  uint32_t keyframe;               /* DELTA: 1 if there was no valid retained copy (every block sent) */
  uint32_t blocks, blocks_total;   /* DELTA: blocks sent / blocks of the rect */
  int32_t  damage[4];              /* DELTA: x, y, w, h (relative to the rect) bounding the sent blocks, each cut to the rect; 0,0,0,0 if none */
  uint64_t bytes;                  /* bytes that crossed to the host for this ticket (header + payload) */
  int32_t  scaled_w, scaled_h;     /* WrhipGrabTextureScaled: the delivered size; 0 for other grabs */
  uint32_t levels;                 /* WrhipGrabTextureScaled: L, the 2:1 steps below the top step */
  uint32_t renditions;             /* WrhipGrabTextureYuvScaled: n, the levels delivered; 0 for other grabs */
  int32_t  scroll_dy;              /* WRHIP_GRAB_SCROLL: the scroll vector (header word 1); 0 for other grabs and for a keyframe */
  uint32_t copied;                 /* WRHIP_GRAB_SCROLL: the COPY entries among `blocks`; 0 for other grabs */
} WrhipGrabInfo;
int32_t WrhipGrabTexture(GLuint tex, const int32_t* rects, int32_t nrects, uint32_t flags);
int32_t WrhipGrabTextureScaled(GLuint tex, const int32_t rect[4], int32_t dst_w, int32_t dst_h, uint32_t flags);
typedef struct WrhipTensorDesc {
  void*    dst;                    /* device memory of this process: WrhipDeviceAlloc'd, or any pointer valid for the context's HIP runtime */
  uint64_t dst_bytes;              /* bytes the library may write from dst on; the extent of the elements must fit */
  int32_t  out_w, out_h;           /* the rect's size: no scaling; smaller: WrhipGrabTextureScaled's chain to out_w x out_h */
  uint32_t dtype, layout, channels;      /* channels: 3 or 4 for GL_RGBA8, 1 for GL_R8 */
  int64_t  row_stride, plane_stride;     /* in ELEMENTS; 0: tight */
  float    scale[4], bias[4];      /* per OUTPUT channel; ignored for U8 */
  uint32_t flags;                  /* WRHIP_GRAB_FLIP_ROWS and / or WRHIP_TENSOR_BGR */
} WrhipTensorDesc;
int32_t WrhipGrabTextureTensor(GLuint tex, const int32_t rect[4], const WrhipTensorDesc* desc);
void* WrhipDeviceAlloc(uint64_t bytes);
void WrhipDeviceFree(void* p);
int32_t WrhipDeviceRead(void* dst_host, const void* src_dev, uint64_t bytes);
int32_t WrhipDeviceWrite(void* dst_dev, const void* src_host, uint64_t bytes);
typedef struct WrhipTensorSrc {
  const void* src;                 /* device memory of this process: WrhipDeviceAlloc'd, or any pointer valid for the context's HIP runtime */
  uint64_t src_bytes;              /* bytes the library may read from src on; the extent of the elements must fit */
  uint32_t dtype, layout, channels;      /* WRHIP_TENSOR_*; channels: 3 or 4 for GL_RGBA8, 1 for GL_R8, 2 for GL_RG8 */
  int64_t  row_stride, plane_stride;     /* in ELEMENTS; 0: tight */
  float    scale[4], bias[4];      /* per INPUT channel; ignored for U8 */
  uint32_t alpha;                  /* the stored A byte (0..255) when channels == 3 */
  uint32_t flags;                  /* WRHIP_GRAB_FLIP_ROWS and / or WRHIP_TENSOR_BGR */
} WrhipTensorSrc;
int32_t WrhipPutTextureTensor(GLuint tex, const int32_t rect[4], const WrhipTensorSrc* desc);
#define WRHIP_PUT_PAYLOAD_LAUNCHES 2   /* most launches of one payload put: the COPY pass, then the patch pass */
int32_t WrhipPutTexturePayload(GLuint tex, const int32_t rect[4], const void* payload, uint64_t bytes, uint32_t flags);
typedef struct WrhipYuvDesc {
  uint32_t format;                 /* WRHIP_YUV_* */
  uint32_t color_space;            /* YuvRangedColorSpace 0..5: Rec601Narrow, Rec601Full, Rec709Narrow, Rec709Full, Rec2020Narrow, Rec2020Full */
  uint32_t flags;                  /* 0 or WRHIP_GRAB_FLIP_ROWS */
  void*    dst;                    /* NULL: planes go to the host through the ticket ring; else device memory */
  uint64_t dst_bytes;              /* device sink: bytes the library may write from dst on */
  int64_t  y_stride, c_stride;     /* device sink, BYTES per row of the Y plane / of a chroma plane; 0: tight */
} WrhipYuvDesc;
int32_t WrhipGrabTextureYuv(GLuint tex, const int32_t rect[4], const WrhipYuvDesc* desc);
int32_t WrhipGrabTextureYuvDelta(GLuint tex, const int32_t rect[4], const WrhipYuvDesc* desc, uint32_t flags);
int32_t WrhipGrabTextureYuvScaled(GLuint tex, const int32_t rect[4], int32_t out_w, int32_t out_h, const WrhipYuvDesc* descs, int32_t renditions);
int32_t WrhipGrabDecodeYuv(const void* payload, uint64_t bytes, uint32_t format, int32_t rect_w, int32_t rect_h, void* y, int64_t y_stride, void* c0, void* c1, int64_t c_stride, int32_t damage[4], uint32_t* blocks);
int32_t WrhipGrabResultGet(int32_t ticket, WrhipGrabInfo* info, void* dst, int64_t dst_stride, int32_t wait);
int32_t WrhipGrabPayloadGet(int32_t ticket, void* dst, uint64_t capacity, uint64_t* bytes, int32_t wait);
int32_t WrhipGrabDecode(const void* payload, uint64_t bytes, uint32_t format, uint32_t flags, int32_t rect_w, int32_t rect_h, void* dst, int64_t dst_stride, int32_t damage[4], uint32_t* blocks);

#ifdef __cplusplus
}
#endif
#endif /* WRHIP_H */
