/* shred_ref.c -- the reference's own shred parse and FEC resolver behind two
   calls, so the shred tests can record what the reference itself decides
   about a buffer.  Built by `make ref REF=<reference tree>` into
   oracle/_ref/libshred_ref.so (never committed); the reference's sources are
   compiled next to this file, nothing of them is restated here.

     shred_ref_parse(buf, sz)                 1 if fd_shred_parse accepts, else 0
     shred_ref_add(buf, sz, pubkey, version)  the raw return value of
                                              fd_fec_resolver_add_shred on a
                                              fresh resolver, SHRED_REF_NO_PARSE
                                              if the parse fails (the shred tile
                                              would not call the resolver), or
                                              SHRED_REF_NO_RESOLVER */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "ballet/shred/fd_shred.h"
#include "ballet/shred/fd_fec_set.h"
#include "disco/shred/fd_fec_resolver.h"
#include "disco/metrics/fd_metrics.h"

#define SHRED_REF_NO_PARSE    (-100)
#define SHRED_REF_NO_RESOLVER (-101)
#define SHRED_REF_BUF_SZ      2048UL   /* room for any packet the callers feed (sz <= 2048) */
#define SHRED_REF_SET_CNT     3UL      /* depth + partial_depth + complete_depth */

/* The three logging hooks the reference's sources call; nothing else of its
   logging is linked. */
long fd_log_wallclock( void ) { return 0L; }

char const * fd_log_private_0( char const * fmt, ... ) { return fmt; }

void fd_log_private_1( int level, long now, char const * file, int line, char const * func, char const * msg ) {
  (void)level; (void)now; (void)file; (void)line; (void)func; (void)msg;
}

void fd_log_private_2( int level, long now, char const * file, int line, char const * func, char const * msg ) {
  (void)level; (void)now;
  fprintf( stderr, "shred_ref: fatal log at %s:%d %s: %s\n", file, line, func, msg );
  abort();
}

static uchar        resolver_mem[ 1UL<<20 ] __attribute__((aligned(FD_FEC_RESOLVER_ALIGN)));
static uchar        shred_mem[ SHRED_REF_SET_CNT*(FD_REEDSOL_DATA_SHREDS_MAX+FD_REEDSOL_PARITY_SHREDS_MAX)*SHRED_REF_BUF_SZ ];
static uchar        metrics_mem[ FD_METRICS_FOOTPRINT( 0, 0 ) ] __attribute__((aligned(FD_METRICS_ALIGN)));
static uchar        packet[ SHRED_REF_BUF_SZ ] __attribute__((aligned(64)));
static fd_fec_set_t sets[ SHRED_REF_SET_CNT ];

int shred_ref_parse( uchar const * buf, ulong sz ) {
  if( sz>SHRED_REF_BUF_SZ ) return 0;
  memset( packet, 0, sizeof(packet) );
  memcpy( packet, buf, sz );
  return !!fd_shred_parse( packet, sz );
}

int shred_ref_add( uchar const * buf, ulong sz, uchar const * leader_pubkey, ushort expected_version ) {
  if( sz>SHRED_REF_BUF_SZ ) return SHRED_REF_NO_PARSE;
  memset( packet, 0, sizeof(packet) );
  memcpy( packet, buf, sz );
  fd_shred_t const * shred = fd_shred_parse( packet, sz );
  if( !shred ) return SHRED_REF_NO_PARSE;

  fd_metrics_register( (ulong *)fd_metrics_new( metrics_mem, 0UL, 0UL ) );

  memset( sets, 0, sizeof(sets) );
  uchar * p = shred_mem;
  for( ulong s=0UL; s<SHRED_REF_SET_CNT; s++ ) {
    for( ulong j=0UL; j<FD_REEDSOL_DATA_SHREDS_MAX;   j++ ) { sets[ s ].data_shreds  [ j ] = p; p += SHRED_REF_BUF_SZ; }
    for( ulong j=0UL; j<FD_REEDSOL_PARITY_SHREDS_MAX; j++ ) { sets[ s ].parity_shreds[ j ] = p; p += SHRED_REF_BUF_SZ; }
  }

  if( fd_fec_resolver_footprint( 1UL, 1UL, 1UL, 1UL )>sizeof(resolver_mem) ) return SHRED_REF_NO_RESOLVER;
  void * formatted = fd_fec_resolver_new( resolver_mem, NULL, NULL, 1UL, 1UL, 1UL, 1UL, sets, expected_version );
  if( !formatted ) return SHRED_REF_NO_RESOLVER;           /* e.g. expected_version 0 */
  fd_fec_resolver_t * resolver = fd_fec_resolver_join( formatted );
  if( !resolver ) return SHRED_REF_NO_RESOLVER;

  fd_fec_set_t const * out_set   = NULL;
  fd_shred_t   const * out_shred = NULL;
  int rv = fd_fec_resolver_add_shred( resolver, shred, sz, leader_pubkey, &out_set, &out_shred );
  fd_fec_resolver_delete( fd_fec_resolver_leave( resolver ) );
  return rv;
}
